"""Fixed-base tables and k_table_msm's fixed plan (csrc/kernels_fixed.h) against the CPU oracle, bit for bit.  Needs an MI355X.

Every expected value comes from the oracle (C.msm_bucket / O.g1_mul / O.g1_add), never from another path of the product: a table of
133 oracle-made points at every term count, batches of uneven MSMs, the callers' skewed scalar patterns, identity / repeated /
opposite / equal / out-of-subgroup bases, the device-resident outputs, the reference prover's recorded halving rounds through
`ipa_rounds(..., table=)`, and the life cycle of the tables."""
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
def pts133():
    rng = random.Random(1330)
    return [O.g1_mul(O.G1_GEN, rng.randint(1, O.R - 1)) for _ in range(133)]


@pytest.fixture(scope="module")
def tab133(ctx, pts133):
    t = ctx.fixed_table(b"".join(raw96(p) for p in pts133), 133)
    assert t.nbytes == 133 * 512 * 1024
    yield t
    t.free()


def s32(values):
    return b"".join(v.to_bytes(32, "little") for v in values)


def neg(pt):
    return None if pt is None else (pt[0], (O.P - pt[1]) % O.P)


def want48(pts, idx, sc):
    """The oracle's compressed sum of sc[i] * pts[idx[i]] (bit 31 of an index = the negated base)."""
    p96 = b"".join(raw96(neg(pts[i & ~NEG]) if i & NEG else pts[i]) for i in idx)
    return C.compress(C.msm_bucket(p96, s32(sc), len(idx))) if idx else O.g1_compress(None)


def got48(ctx, tab, idx, sc, offsets=None):
    offsets = [0, len(idx)] if offsets is None else offsets
    out = ctx.fixed_msm_host(tab, idx, s32(sc), offsets, compressed=True)
    return out[0] if len(offsets) == 2 else out


def compress_blob(N, blob):
    out = ctypes.create_string_buffer(48)
    N.cg1_compress(out, blob)
    return out.raw


def test_every_term_count(native_lib, ctx, tab133, pts133):
    rng = random.Random(1331)
    for n in list(range(1, 301)) + [512, 627, 1024, 2048]:
        idx = [rng.randrange(133) for _ in range(n)]
        sc = [rng.randrange(O.R) for _ in range(n)]
        assert got48(ctx, tab133, idx, sc) == want48(pts133, idx, sc), n
    # the blob output is the same point
    idx, sc = [5, 7, 5], [3, 4, O.R - 2]
    blob = ctx.fixed_msm_host(tab133, idx, s32(sc), [0, 3])[0]
    assert compress_blob(native_lib, blob) == want48(pts133, idx, sc)


@pytest.mark.parametrize("m", [1, 4, 7, 64, 256])
def test_msm_many_uneven(ctx, tab133, pts133, m):
    rng = random.Random(1332 + m)
    lens = [rng.choice([0, 0, 1, 2, 7, 8, 9, 15, 16, 17, 33, 65, 65, 124, 133, 300]) for _ in range(m)]
    if m >= 4:
        lens[0], lens[-1], lens[m // 2] = 0, 0, 700                  # empty MSMs at both ends, one far longer than the rest
    idx, sc, offsets = [], [], [0]
    for n in lens:
        idx += [rng.randrange(133) | (NEG if rng.random() < 0.2 else 0) for _ in range(n)]
        sc += [rng.randrange(O.R) for _ in range(n)]
        offsets.append(len(idx))
    got = ctx.fixed_msm_host(tab133, idx, s32(sc), offsets, compressed=True)
    assert len(got) == m
    for j in range(m):
        a, b = offsets[j], offsets[j + 1]
        assert got[j] == want48(pts133, idx[a:b], sc[a:b]), (m, j, lens[j])


def test_limits(native_lib, ctx, tab133):
    N = native_lib
    with pytest.raises(N.NativeError):
        ctx.fixed_msm_host(tab133, [0] * (N.FIXED_MAX_TERMS + 1), s32([1] * (N.FIXED_MAX_TERMS + 1)), [0, N.FIXED_MAX_TERMS + 1])
    with pytest.raises(N.NativeError):
        ctx.fixed_msm_host(tab133, [], b"", [0] * (N.FIXED_MAX_MSMS + 2))
    with pytest.raises(N.NativeError):
        ctx.fixed_msm_host(tab133, [133], s32([1]), [0, 1])              # index outside the table
    st = ctypes.c_int(0)
    assert not N.cg1_fixed_create(ctx.handle, bytes(96 * (N.FIXED_MAX_BASES + 1)), N.FIXED_MAX_BASES + 1, ctypes.byref(st)) and st.value == N.ERR_ARG
    bad = (O.P).to_bytes(48, "little") + (2).to_bytes(48, "little")      # x = p: not canonical
    assert not N.cg1_fixed_create(ctx.handle, bad, 1, ctypes.byref(st)) and st.value == N.ERR_ENCODING
    off = (1).to_bytes(48, "little") + (1).to_bytes(48, "little")        # 1 != 1 + 4: off the curve
    assert not N.cg1_fixed_create(ctx.handle, off, 1, ctypes.byref(st)) and st.value == N.ERR_NOT_ON_CURVE


def test_scalar_patterns(native_lib, ctx, tab133, pts133):
    N = native_lib
    rng = random.Random(1340)
    for n in (1, 65, 124, 133, 300):
        idx = list(range(n)) if n <= 133 else [rng.randrange(133) for _ in range(n)]
        k = rng.randrange(O.R)
        for name, sc in (("equal", [k] * n), ("sigma", list(range(n))), ("r-1", [O.R - 1] * n), ("zeros", [0] * n),
                         ("one hot", [0] * (n - 1) + [k])):
            assert got48(ctx, tab133, idx, sc) == want48(pts133, idx, sc), (name, n)
    assert got48(ctx, tab133, [3] * 4, [0] * 4) == O.g1_compress(None)
    # a scalar >= r: the documented error for the whole call, nothing written
    for bad in (O.R, O.R + 1, (1 << 256) - 1):
        idx, sc, offsets = [1, 2, 3, 4], [5, 6, bad, 7], [0, 2, 4]
        tb = (ctypes.c_uint32 * 4)(*idx)
        offs = (ctypes.c_uint32 * 3)(*offsets)
        blobs = ctypes.create_string_buffer(b"\xaa" * (2 * N.POINT_BYTES), 2 * N.POINT_BYTES)
        comp = ctypes.create_string_buffer(b"\xaa" * 96, 96)
        assert N.cg1_fixed_msm(ctx.handle, tab133.handle, tb, s32(sc), offs, 2, blobs, comp) == N.ERR_ENCODING
        assert blobs.raw == b"\xaa" * (2 * N.POINT_BYTES) and comp.raw == b"\xaa" * 96
        with pytest.raises(N.NativeError):
            ctx.fixed_msm_host(tab133, idx, s32(sc), offsets)
    assert got48(ctx, tab133, [1, 2], [5, 6]) == want48(pts133, [1, 2], [5, 6])       # the table works on after a refused call


def test_base_patterns(native_lib, ctx, pts133):
    rng = random.Random(1350)
    tors = json.load(open(os.path.join(ROOT, "tests", "golden", "torsion_vectors.json")))
    T3 = O.g1_decompress(bytes.fromhex(tors["t3"]))
    assert T3 == (0, 2) and O.g1_is_on_curve(T3) and not O.g1_in_subgroup(T3)
    mixed = O.g1_add(T3, pts133[9])                                      # order 3 r: outside G1, not of small order
    # 0: identity   1, 2: equal points   3: T3   4: T3 + P   5 ..: ordinary points
    pts = [None, pts133[0], pts133[0], T3, mixed] + pts133[1:8]
    tab = ctx.fixed_table(b"".join(raw96(p) for p in pts), len(pts))
    try:
        k = rng.randrange(O.R)
        assert got48(ctx, tab, [0], [k]) == O.g1_compress(None)                              # the identity base
        assert got48(ctx, tab, [0, 5, 0], [k, 7, 1]) == want48(pts, [0, 5, 0], [k, 7, 1])
        for n in (2, 40, 700):                                                                # the same index many times
            sc = [rng.randrange(O.R) for _ in range(n)]
            assert got48(ctx, tab, [6] * n, sc) == O.g1_compress(O.g1_mul(pts[6], sum(sc) % O.R)), n
            assert got48(ctx, tab, [6] * n, [k] * n) == O.g1_compress(O.g1_mul(pts[6], k * n % O.R)), n
        assert got48(ctx, tab, [7, 7 | NEG], [k, k]) == O.g1_compress(None)                   # k B + k (-B)
        assert got48(ctx, tab, [7, 8, 7 | NEG], [k, 3, k]) == O.g1_compress(O.g1_mul(pts[8], 3))
        assert got48(ctx, tab, [7 | NEG], [k]) == O.g1_compress(O.g1_mul(neg(pts[7]), k))
        assert got48(ctx, tab, [1, 2], [k, k]) == O.g1_compress(O.g1_mul(pts[1], 2 * k % O.R))   # two table bases that are equal points: P + P
        assert got48(ctx, tab, [1, 2 | NEG], [k, k]) == O.g1_compress(None)
        # bases outside G1: k P depends on the INTEGER k -- the oracle's multiplication takes k < r as it is
        for kk in (1, 2, 3, 4, 5, 255, 256, 257, O.R - 1, O.R - 2, k, rng.randrange(O.R)):
            assert kk < O.R
            assert got48(ctx, tab, [3], [kk]) == O.g1_compress(O.g1_mul(T3, kk)), kk
            assert got48(ctx, tab, [4], [kk]) == O.g1_compress(O.g1_mul(mixed, kk)), kk
        assert O.g1_mul(T3, O.R - 1) is None and O.g1_mul(T3, O.R - 2) is not None           # r = 1 (mod 3): the integer matters
        sc = [rng.randrange(O.R) for _ in range(6)]
        idx = [3, 4, 5, 3 | NEG, 4, 6]
        want = None
        for i, v in zip(idx, sc):
            b = pts[i & ~NEG]
            want = O.g1_add(want, O.g1_mul(neg(b) if i & NEG else b, v))
        assert got48(ctx, tab, idx, sc) == O.g1_compress(want)
    finally:
        tab.free()


def test_device_entry_equals_host_entry(native_lib, ctx, tab133, pts133):
    rng = random.Random(1360)
    lens = [0, 1, 65, 65, 9, 0, 300, 133, 16, 17, 2048, 3]
    idx, sc, offsets = [], [], [0]
    for n in lens:
        idx += [rng.randrange(133) | (NEG if rng.random() < 0.3 else 0) for _ in range(n)]
        sc += [rng.randrange(O.R) for _ in range(n)]
        offsets.append(len(idx))
    m, nt = len(lens), len(idx)
    host = ctx.fixed_msm_host(tab133, idx, s32(sc), offsets, compressed=True)
    for j in range(m):
        assert host[j] == want48(pts133, idx[offsets[j]:offsets[j + 1]], sc[offsets[j]:offsets[j + 1]]), j
    d_tb, d_sc, d_off = ctx.alloc(4 * nt), ctx.alloc(32 * nt), ctx.alloc(4 * (m + 1))
    d_a, d_k = ctx.alloc(96 * m), ctx.alloc(48 * m)
    d_tb.upload(b"".join(i.to_bytes(4, "little") for i in idx)); d_sc.upload(s32(sc)); d_off.upload(b"".join(o.to_bytes(4, "little") for o in offsets))
    try:
        for outs in ((d_a, d_k), (d_a, None), (None, d_k)):
            d_a.upload(b"\x55" * (96 * m)); d_k.upload(b"\x55" * (48 * m))
            ctx.fixed_msm_device(tab133, d_tb, d_sc, d_off, m, nt, max(lens), outs[0], outs[1])
            if outs[1] is not None:
                k48 = d_k.download()
                assert [k48[48 * j: 48 * j + 48] for j in range(m)] == host
            if outs[0] is not None:
                a96 = d_a.download()
                for j in range(m):
                    rec = a96[96 * j: 96 * j + 96]
                    assert C.compress(rec) == host[j], j
        # a scalar >= r among the device arrays: the documented error, outputs untouched
        bad = list(sc); bad[70] = O.R
        d_sc.upload(s32(bad))
        d_a.upload(b"\x55" * (96 * m)); d_k.upload(b"\x55" * (48 * m))
        with pytest.raises(native_lib.NativeError):
            ctx.fixed_msm_device(tab133, d_tb, d_sc, d_off, m, nt, max(lens), d_a, d_k)
        assert d_a.download() == b"\x55" * (96 * m) and d_k.download() == b"\x55" * (48 * m)
        d_sc.upload(s32(sc))
        ctx.fixed_msm_device(tab133, d_tb, d_sc, d_off, m, nt, max(lens), None, d_k)          # and the table works on
        k48 = d_k.download()
        assert [k48[48 * j: 48 * j + 48] for j in range(m)] == host
    finally:
        for b in (d_tb, d_sc, d_off, d_a, d_k):
            b.free()


# ---- the Python class and the prover's halving rounds

def P(h):
    from curdleproofs_pie_amd.py_arkworks_bls12381 import G1Point
    return G1Point.from_compressed_bytes_unchecked(bytes.fromhex(h))


def S(h):
    from curdleproofs_pie_amd.py_arkworks_bls12381 import Scalar
    return Scalar.from_le_bytes(bytes.fromhex(h))


def enc(points):
    return [bytes(p.to_compressed_bytes()).hex() for p in points]


@pytest.fixture(scope="module")
def ipa_vectors(native_lib):
    r = json.load(open(os.path.join(ROOT, "tests", "golden", "prover_vectors.json")))["ipa"]
    x = json.load(open(os.path.join(ROOT, "tests", "golden", "fixed_base_vectors.json")))
    assert x["H"] == r["H"]
    crs_H, beta = O.g1_decompress(bytes.fromhex(x["ipa_crs_H"])), int.from_bytes(bytes.fromhex(x["ipa_beta"]), "little")
    assert O.g1_compress(O.g1_mul(crs_H, beta)).hex() == r["H"]          # the new fixture belongs to the recorded run
    return r, x


def mk_gammas(r):
    gs = [S(g) for g in r["gammas"]]
    return lambda *pts: gs.pop(0)


def test_python_class(native_lib, pts133):
    from curdleproofs_pie_amd import G1Point, Scalar
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable

    objs = [G1Point.from_compressed_bytes_unchecked(O.g1_compress(p)) for p in pts133[:40]]
    objs.append(objs[3] * Scalar(77) + objs[4])                           # a deferred value: forced by the constructor
    pts = pts133[:40] + [O.g1_add(O.g1_mul(pts133[3], 77), pts133[4])]
    tab = FixedBaseTable(objs)
    try:
        assert len(tab) == 41 and tab.nbytes == 41 * 512 * 1024
        assert tab.index(objs[7]) == 7 and tab.index(objs[40]) == 40
        with pytest.raises(KeyError):
            tab.index(G1Point.from_compressed_bytes_unchecked(O.g1_compress(pts133[7])))      # an equal point, another object
        rng = random.Random(1370)
        sc = [rng.randrange(O.R) for _ in range(41)]
        assert bytes(tab.msm([Scalar(v) for v in sc]).to_compressed_bytes()) == want48(pts, list(range(41)), sc)
        assert bytes(tab.msm([Scalar(v) for v in sc[:5]]).to_compressed_bytes()) == want48(pts, list(range(5)), sc[:5])
        sel = [40, 3, 3, 17]
        assert bytes(tab.msm([Scalar(v) for v in sc[:4]], [objs[i] for i in sel]).to_compressed_bytes()) == want48(pts, sel, sc[:4])
        assert bytes(tab.msm([Scalar(v) for v in sc[:4]], sel).to_compressed_bytes()) == want48(pts, sel, sc[:4])
        jobs = [([objs[1], 2], [Scalar(5), Scalar(6)]), ([], []), (None, [Scalar(v) for v in sc])]
        got = tab.msm_many(jobs)
        assert [bytes(g.to_compressed_bytes()) for g in got] == [want48(pts, [1, 2], [5, 6]), O.g1_compress(None), want48(pts, list(range(41)), sc)]
        assert tab.msm_many([]) == []
        with pytest.raises(KeyError):
            tab.msm([Scalar(1)], [G1Point()])
        with pytest.raises(IndexError):
            tab.msm([Scalar(1)], [41])
    finally:
        tab.close()
    assert tab.nbytes == 0
    with pytest.raises(native_lib.NativeError):
        tab.msm([Scalar(1)])
    tab.close()                                                            # closing twice is harmless


def test_ipa_rounds_with_table_reproduce_reference_bytes(ipa_vectors):
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.prover_kernels import ipa_rounds, ipa_rounds_many

    r, x = ipa_vectors
    G, Gp, H = [P(h) for h in r["crs_G_vec"]], [P(h) for h in r["crs_G_prime_vec"]], P(r["H"])
    c, d = [S(h) for h in r["vec_c"]], [S(h) for h in r["vec_d"]]
    want = (r["vec_L_C"], r["vec_R_C"], r["vec_L_D"], r["vec_R_D"])
    tab = FixedBaseTable(G + Gp + [H])
    try:
        LC, RC, LD, RD, c_fin, d_fin = ipa_rounds(G, Gp, H, c, d, mk_gammas(r), table=tab)
        assert (enc(LC), enc(RC), enc(LD), enc(RD)) == want
        assert bytes(c_fin.to_le_bytes()).hex() == r["c_final"] and bytes(d_fin.to_le_bytes()).hex() == r["d_final"]
        # three provers in step: prover 0 is the recorded one, the others' vectors are rotated; each equals what it gets alone
        rot = lambda v, k: v[k:] + v[:k]
        provers = [(G, Gp, H, c, d)] + [(G, Gp, H, rot(c, k), rot(d, 2 * k)) for k in (1, 2)]
        many = ipa_rounds_many(provers, [mk_gammas(r) for _ in provers], table=tab)
        assert tuple(enc(v) for v in many[0][:4]) == want
        assert bytes(many[0][4].to_le_bytes()).hex() == r["c_final"] and bytes(many[0][5].to_le_bytes()).hex() == r["d_final"]
        for pr, got in zip(provers[1:], many[1:]):
            alone = ipa_rounds(*pr, mk_gammas(r))                          # without a table: compute_MSM_batch
            assert [enc(v) for v in got[:4]] == [enc(v) for v in alone[:4]] and got[4] == alone[4] and got[5] == alone[5]
        with pytest.raises(KeyError):                                      # a base that is not an object of the table
            ipa_rounds(G, Gp, P(r["H"]), c, d, mk_gammas(r), table=tab)
    finally:
        tab.close()


def test_ipa_rounds_with_crs_H_and_coefficient(ipa_vectors):
    """`H` = crs_H * beta is not a CRS point: the table holds crs_H, the prover passes beta as H_coeff."""
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.prover_kernels import ipa_rounds

    r, x = ipa_vectors
    G, Gp, crs_H, beta = [P(h) for h in r["crs_G_vec"]], [P(h) for h in r["crs_G_prime_vec"]], P(x["ipa_crs_H"]), S(x["ipa_beta"])
    c, d = [S(h) for h in r["vec_c"]], [S(h) for h in r["vec_d"]]
    tab = FixedBaseTable(G + Gp + [crs_H])
    try:
        LC, RC, LD, RD, c_fin, d_fin = ipa_rounds(G, Gp, crs_H, c, d, mk_gammas(r), H_coeff=beta, table=tab)
        assert (enc(LC), enc(RC), enc(LD), enc(RD)) == (r["vec_L_C"], r["vec_R_C"], r["vec_L_D"], r["vec_R_D"])
        assert bytes(c_fin.to_le_bytes()).hex() == r["c_final"] and bytes(d_fin.to_le_bytes()).hex() == r["d_final"]
    finally:
        tab.close()
    # the coefficient alone (no table) gives the same bytes through compute_MSM_batch
    LC, RC, LD, RD, _, _ = ipa_rounds(G, Gp, crs_H, c, d, mk_gammas(r), H_coeff=beta)
    assert (enc(LC), enc(RC), enc(LD), enc(RD)) == (r["vec_L_C"], r["vec_R_C"], r["vec_L_D"], r["vec_R_D"])


def test_permute_and_commit_with_table(native_lib, monkeypatch):
    import curdleproofs_pie_amd.prover_kernels as K
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable

    pv = json.load(open(os.path.join(ROOT, "tests", "golden", "prover_vectors.json")))
    r, g = pv["permute_commit"], pv["grand_product_bases"]
    blinders = [S(b) for b in r["blinders"]]
    monkeypatch.setattr(K, "random_scalar", lambda: blinders.pop(0))

    class Crs:
        pass

    crs = Crs()
    crs.vec_G, crs.vec_H = [P(h) for h in g["vec_G"]], [P(h) for h in g["vec_H"]]
    tab = FixedBaseTable(crs.vec_G + crs.vec_H)
    try:
        vec_T, vec_U, M, bl = K.shuffle_permute_and_commit_input(crs, [P(h) for h in r["vec_R"]], [P(h) for h in r["vec_S"]], r["permutation"], S(r["k"]), table=tab)
    finally:
        tab.close()
    assert enc(vec_T) == r["vec_T"] and enc(vec_U) == r["vec_U"] and enc([M]) == [r["M"]]


def test_two_tables_and_close(native_lib, ctx, pts133):
    """Two tables alive on one context do not interfere; a closed table raises instead of reading freed memory; the tables of the
    default context are freed before it closes."""
    from curdleproofs_pie_amd import G1Point, Scalar
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable

    N = native_lib
    rng = random.Random(1380)
    a_pts, b_pts = pts133[:20], pts133[50:90]
    ta = ctx.fixed_table(b"".join(raw96(p) for p in a_pts), 20)
    tb = ctx.fixed_table(b"".join(raw96(p) for p in b_pts), 40)
    for _ in range(6):
        for tab, pts in ((ta, a_pts), (tb, b_pts), (tb, b_pts), (ta, a_pts)):
            n = rng.randrange(1, 400)
            idx = [rng.randrange(len(pts)) for _ in range(n)]
            sc = [rng.randrange(O.R) for _ in range(n)]
            assert got48(ctx, tab, idx, sc) == want48(pts, idx, sc)
    ta.free()
    with pytest.raises(N.NativeError):
        ctx.fixed_msm_host(ta, [0], s32([1]), [0, 1])
    assert got48(ctx, tb, [1, 2], [3, 4]) == want48(b_pts, [1, 2], [3, 4])           # the other one lives on
    tb.free()
    objs = [G1Point.from_compressed_bytes_unchecked(O.g1_compress(p)) for p in pts133[:3]]
    t = FixedBaseTable(objs)
    assert bytes(t.msm([Scalar(2), Scalar(3), Scalar(4)]).to_compressed_bytes()) == want48(pts133, [0, 1, 2], [2, 3, 4])
    N.close_default_context()                                                          # frees the table first
    assert t.nbytes == 0
    with pytest.raises(N.NativeError):
        t.msm([Scalar(1)])
    t2 = FixedBaseTable(objs)                                                          # a new default context, a new table
    assert bytes(t2.msm([Scalar(2), Scalar(3), Scalar(4)]).to_compressed_bytes()) == want48(pts133, [0, 1, 2], [2, 3, 4])
    t2.close()
