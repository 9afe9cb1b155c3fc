"""prover_kernels.same_scalar_prove_device / cg1_same_scalar_prove_device (csrc/kernels_same_scalar.h): the shuffle prover's same-scalar
block -- R, S, cm_T, cm_U and all of SameScalarProof.new -- as one launch chain over ONE light table of G_t | G_u | H | vec_R | vec_S built
inside the call.  Needs an MI355X.

Pinned to the reference's bytes: tests/golden/same_scalar_device_vectors.json records curdleproofs.py:92-116 run stand-alone (the 576
bytes, and a challenge drawn afterwards that pins the final transcript state).  Both settings of bases_certified give them; provers in
step must each get what they get alone; edge inputs are compared with a host-driven path that multiplies R itself (eager operators, the
host transcript, Python ints); a base outside G1 and every other refusal leave the outputs and the transcript alone; and the chain shares
one table handle -- staging block, light-table scratch -- with the other three device provers."""
import ctypes
import json
import os
import random
import sys

import pytest

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu
R = O.R
INF = b"\xc0" + bytes(47)
NOT_G1_TEXT = "outside the prime-order subgroup"


def P(h):
    """Decoded unchecked: membership in G1 not known."""
    from curdleproofs_pie_amd.py_arkworks_bls12381 import G1Point
    return G1Point.from_compressed_bytes_unchecked(bytes.fromhex(h) if isinstance(h, str) else h)


def Pc(h):
    """Decoded checked: carries its membership certificate."""
    from curdleproofs_pie_amd.py_arkworks_bls12381 import G1Point
    return G1Point.from_compressed_bytes(bytes.fromhex(h) if isinstance(h, str) else h)


def S(h):
    from curdleproofs_pie_amd.py_arkworks_bls12381 import Scalar
    return Scalar.from_le_bytes(bytes.fromhex(h))


def fr32(s):
    return bytes(s.to_le_bytes())


def golden(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))["cases"]


@pytest.fixture(scope="module")
def cases(native_lib):
    return golden("same_scalar_device_vectors.json")


class Case:
    """A fixture case as product objects.  The chain's home is a FixedBaseTable over the three CRS points (any table would do)."""

    def __init__(self, case, decode=P, own_table=True):
        from curdleproofs_pie_amd.fixed_base import FixedBaseTable

        self.raw, self.ell = case, case["ell"]
        ell = self.ell
        if "vec_R" in case:
            self.Gt, self.Gu, self.H = decode(case["crs_G_t"]), decode(case["crs_G_u"]), decode(case["crs_H"])
            self.vR, self.vS = [decode(h) for h in case["vec_R"]], [decode(h) for h in case["vec_S"]]
        else:                                                            # not stored: G1 * k, the 2 ell + 3 scalars k the case's seed gives first
            from curdleproofs_pie_amd import G1Point, Scalar
            from curdleproofs_pie_amd.msm_accumulator import batch_mul

            rng = random.Random(case["seed"])
            pts = batch_mul([G1Point()] * (2 * ell + 3), [Scalar(rng.randint(1, R - 1)) for _ in range(2 * ell + 3)])
            pts = [decode(bytes(p.to_compressed_bytes())) for p in pts]
            self.Gt, self.Gu, self.H, self.vR, self.vS = pts[0], pts[1], pts[2], pts[3: 3 + ell], pts[3 + ell:]
        self.a, self.k = [S(h) for h in case["vec_a"]], S(case["k"])
        self.bl = [S(case[key]) for key in ("r_t", "r_u", "r_a", "r_b", "r_k")]
        self.table = FixedBaseTable([self.Gt, self.Gu, self.H]) if own_table else None

    def transcript(self, prefix=None):
        from curdleproofs_pie_amd.merlin import CurdleproofsTranscript

        t = CurdleproofsTranscript(self.raw["label"].encode())
        t.append(self.raw["prefix_label"].encode(), bytes.fromhex(self.raw["prefix"]) if prefix is None else prefix)
        return t

    def prover(self, rot=0):
        """Prover `rot` of a call in step: rotated vec_a, vec_R and vec_S (S reversed for odd rot), its own k and blinders."""
        from curdleproofs_pie_amd import Scalar

        r = lambda v, j: v[j % len(v):] + v[:j % len(v)]
        vS = r(self.vS, 2 * rot)
        if rot % 2:
            vS = vS[::-1]
        bl = [b + Scalar(7 * rot * (i + 1)) for i, b in enumerate(self.bl)]
        return (self.Gt, self.Gu, self.H, r(self.vR, rot), vS, r(self.a, 3 * rot), self.k + Scalar(rot), *bl)


def to_bytes(res):
    """cm_T | cm_U | R | S | cm_A | cm_B | z_k | z_t | z_u."""
    R_, S_, cm_T, cm_U, cm_A, cm_B, z_k, z_t, z_u = res
    comp = lambda p: bytes(p.to_compressed_bytes())
    return b"".join(comp(p) for p in [*cm_T, *cm_U, R_, S_, *cm_A, *cm_B]) + fr32(z_k) + fr32(z_t) + fr32(z_u)


def state(t):
    return bytes(t.strobe._st.raw)


def host_driven(Gt, Gu, H, vR, vS, a, k, r_t, r_u, r_a, r_b, r_k, transcript):
    """curdleproofs.py:92-116 after the draws, driven from the host as the reference writes it: the sums term by term with the eager
    operators, R * k and R * r_k UNFOLDED (R itself is multiplied), the host transcript, the responses in Python ints."""
    from curdleproofs_pie_amd import Scalar

    def msm(points, scalars):
        acc = None
        for p, s in zip(points, scalars):
            acc = p * s if acc is None else acc + p * s
        return acc

    comp = lambda p: bytes(p.to_compressed_bytes())
    R_, S_ = msm(vR, a), msm(vS, a)
    R_, S_ = P(comp(R_)), P(comp(S_))                                    # materialised: what is multiplied below is the point R, not its terms
    commit = lambda G, T, r: (G * r, T + H * r)                          # commitment.py:30
    cm_T, cm_U = commit(Gt, R_ * k, r_t), commit(Gu, S_ * k, r_u)
    cm_A, cm_B = commit(Gt, R_ * r_k, r_a), commit(Gu, S_ * r_k, r_b)
    transcript.append_list(b"sameexp_points", [comp(p) for p in (R_, S_, *cm_T, *cm_U, *cm_A, *cm_B)])
    alpha = int(transcript.get_and_append_challenge(b"same_scalar_alpha"))
    z = [(int(r_k) + int(k) * alpha) % R, (int(r_a) + int(r_t) * alpha) % R, (int(r_b) + int(r_u) * alpha) % R]
    return (R_, S_, cm_T, cm_U, cm_A, cm_B, *(Scalar(v) for v in z))


@pytest.mark.parametrize("certified", [False, True])
@pytest.mark.parametrize("which", range(6))
def test_fixture_cases_reproduce_reference_bytes(cases, which, certified):
    """ell = 1, 2, 5, 8, 28, 124, with the subgroup launch (bases decoded unchecked) and without it (bases that carry their certificate)."""
    from curdleproofs_pie_amd.prover_kernels import same_scalar_prove_device

    k = Case(cases[which], decode=Pc if certified else P)
    try:
        assert all((x._sg is True) == certified for x in k.vR + k.vS)
        a_before = [fr32(s) for s in k.a]
        for _ in range(2):                                               # twice: the same bytes, the same state
            t = k.transcript()
            res = same_scalar_prove_device(k.table, *k.prover(), t)
            assert to_bytes(res).hex() == k.raw["proof"], k.ell
            assert fr32(t.get_and_append_challenge(b"after")).hex() == k.raw["after"]
        assert [fr32(s) for s in k.a] == a_before and all((x._sg is True) == certified for x in k.vR + k.vS)      # nothing mutated, no host test run
        if not certified:
            t3 = k.transcript()                                          # the host-driven path agrees on both
            assert to_bytes(host_driven(*k.prover(), t3)).hex() == k.raw["proof"]
            assert fr32(t3.get_and_append_challenge(b"after")).hex() == k.raw["after"]
    finally:
        k.table.close()


@pytest.mark.parametrize("which", [2, 4])
def test_provers_in_step(cases, which):
    """Batches of 1, 3, 8 and 64 provers at ell = 5 and ell = 28: rotated vectors, own k and blinders, different transcript prefixes;
    prover 0 is the fixture's; every prover's bytes and final state equal what it gets alone."""
    from curdleproofs_pie_amd.prover_kernels import same_scalar_prove_device_many

    k = Case(cases[which])
    assert k.ell in (5, 28)
    try:
        alone = {}
        for batch in (1, 3, 8, 64):
            provers = [k.prover(rot=i) for i in range(batch)]
            prefix = lambda i: None if i == 0 else b"prover %d" % i
            ts = [k.transcript(prefix(i)) for i in range(batch)]
            got = same_scalar_prove_device_many(k.table, provers, ts)
            assert len(got) == batch
            assert to_bytes(got[0]).hex() == k.raw["proof"] and fr32(ts[0].get_and_append_challenge(b"after")).hex() == k.raw["after"]
            for i in range(1, batch):
                if i not in alone:
                    t1 = k.transcript(prefix(i))
                    alone[i] = (to_bytes(same_scalar_prove_device_many(k.table, [provers[i]], [t1])[0]), state(t1))
                assert (to_bytes(got[i]), state(ts[i])) == alone[i], (batch, i)
            assert len({to_bytes(g) for g in got}) == batch
    finally:
        k.table.close()


def test_more_provers_than_one_call_and_other_crs_points(cases):
    """70 provers, the third with another crs_H: calls of 2, 1 (a change of the CRS points starts a call of its own), 64 (the most one call
    carries) and 3 provers.  Each gets what it gets alone."""
    from curdleproofs_pie_amd.prover_kernels import same_scalar_prove_device_many

    k = Case(cases[1])                                                   # ell = 2
    try:
        provers = [k.prover(rot=i) for i in range(70)]
        provers[2] = provers[2][:2] + (k.Gt,) + provers[2][3:]           # crs_H = crs_G_t for prover 2 only
        ts = [k.transcript(b"prover %d" % i) for i in range(70)]
        got = same_scalar_prove_device_many(k.table, provers, ts)
        assert len(got) == 70
        for i in (0, 1, 2, 3, 66, 67, 69):
            t1 = k.transcript(b"prover %d" % i)
            assert (to_bytes(got[i]), state(ts[i])) == (to_bytes(same_scalar_prove_device_many(k.table, [provers[i]], [t1])[0]), state(t1)), i
        t2 = k.transcript(b"prover 2")
        assert to_bytes(got[2]) == to_bytes(host_driven(*provers[2], t2)) and state(ts[2]) == state(t2)
    finally:
        k.table.close()


def test_edge_inputs_against_the_host_driven_path(native_lib):
    """Seeded inputs: identity entries in vec_R; vec_R = [P, -P] with equal a, so R = O; k = 0; r_t = 0, so T_1 = O; repeated points; and
    ell = 300, where a lane owns two elements and an MSM spans several slices -- the device chain and the host-driven path give the same
    bytes and the same transcript."""
    from curdleproofs_pie_amd import G1Point, Scalar
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.merlin import CurdleproofsTranscript
    from curdleproofs_pie_amd.msm_accumulator import batch_mul
    from curdleproofs_pie_amd.prover_kernels import same_scalar_prove_device

    rng = random.Random(9001)
    obj = lambda p: P(O.g1_compress(p))
    rpt = lambda: O.g1_mul(O.G1_GEN, rng.randrange(1, R))
    rs = lambda n: [Scalar(rng.randrange(R)) for _ in range(n)]
    Gt, Gu, H = obj(rpt()), obj(rpt()), obj(rpt())
    tab = FixedBaseTable([Gt, Gu, H])
    n = 6
    Rp, Sp = [rpt() for _ in range(n)], [rpt() for _ in range(n)]
    ids = list(Rp)
    ids[0] = ids[3] = ids[5] = None
    pair = [Rp[0], O.g1_neg(Rp[0])]
    rep = [Rp[0], Rp[1], Rp[0], Rp[0], Rp[1], Sp[2]]
    a_eq = Scalar(rng.randrange(R))
    big = batch_mul([G1Point()] * 600, [Scalar(rng.randrange(1, R)) for _ in range(600)])
    big = [P(bytes(p.to_compressed_bytes())) for p in big]
    o = lambda v: [obj(p) for p in v]
    # name: (vec_R, vec_S, vec_a, k, [r_t, r_u, r_a, r_b, r_k])
    shapes = {
        "identities in vec_R": (o(ids), o(Sp), rs(n), rs(1)[0], rs(5)),
        "all identities": (o([None] * n), o([None] * n), rs(n), rs(1)[0], rs(5)),
        "R = O": (o(pair), o(Sp[:2]), [a_eq, a_eq], rs(1)[0], rs(5)),
        "k = 0": (o(Rp), o(Sp), rs(n), Scalar(0), rs(5)),
        "r_t = 0": (o(Rp), o(Sp), rs(n), rs(1)[0], [Scalar(0)] + rs(4)),
        "all blinders zero": (o(Rp), o(Sp), rs(n), rs(1)[0], [Scalar(0)] * 5),
        "repeated points": (o(rep), o(rep[::-1]), rs(n), rs(1)[0], rs(5)),
        "vec_a zero": (o(Rp), o(Sp), [Scalar(0)] * n, rs(1)[0], rs(5)),
        "ell = 300": (big[:300], big[300:], rs(300), rs(1)[0], rs(5)),
    }
    try:
        for name, (vR, vS, a, k, bl) in shapes.items():
            mk = lambda: CurdleproofsTranscript(b"edge " + name.encode())
            t_dev, t_host = mk(), mk()
            got = same_scalar_prove_device(tab, Gt, Gu, H, vR, vS, a, k, *bl, t_dev)
            want = host_driven(Gt, Gu, H, vR, vS, a, k, *bl, t_host)
            assert to_bytes(got) == to_bytes(want), name
            assert state(t_dev) == state(t_host), name
            raw = to_bytes(got)
            slot = lambda j: raw[48 * j: 48 * j + 48]                    # cm_T | cm_U | R | S | cm_A | cm_B
            if name == "R = O":
                assert slot(4) == INF and slot(5) != INF
            if name == "r_t = 0":
                assert slot(0) == INF and slot(2) != INF
            if name == "all identities":
                assert slot(4) == slot(5) == INF and slot(0) != INF
            if name == "k = 0":                                          # T_2 = r_t H alone
                assert slot(1) == bytes((H * bl[0]).to_compressed_bytes())
    finally:
        tab.close()


def raw_args(k, P_=1):
    """The C entry's arguments for P_ copies of a fixture case."""
    from curdleproofs_pie_amd.py_arkworks_bls12381 import points_to_affine96

    vec = lambda keys: b"".join(bytes.fromhex(k.raw[key]) for key in keys) * P_
    return dict(gth=bytes(points_to_affine96([k.Gt, k.Gu, k.H])), rs=bytes(points_to_affine96(k.vR + k.vS)) * P_,
                a=b"".join(bytes.fromhex(h) for h in k.raw["vec_a"]) * P_, k=vec(["k"]), bl=vec(["r_t", "r_u", "r_a", "r_b", "r_k"]), certified=0)


def call_raw(N, ctx_handle, tab_handle, ell, P_, a, st, out):
    return N.cg1_same_scalar_prove_device(ctx_handle, tab_handle, ell, P_, a["gth"], a["rs"], a["a"], a["k"], a["bl"], a["certified"], st, out, None)


def torsion_point():
    """T3 + P for the order-3 point T3 of tests/golden/torsion_vectors.json: on the curve, of order 3 r, outside G1."""
    tors = json.load(open(os.path.join(ROOT, "tests", "golden", "torsion_vectors.json")))
    T3 = O.g1_decompress(bytes.fromhex(tors["t3"]))
    assert not O.g1_in_subgroup(T3) and O.g1_mul(T3, 3) is None
    pt = O.g1_add(T3, O.g1_mul(O.G1_GEN, 0x5EED))
    assert not O.g1_in_subgroup(pt)
    return pt


def test_a_base_outside_g1_is_refused(native_lib, cases):
    """A vec_R entry T3 + P: refused with the entry's own text, outputs and transcript untouched, and the next valid call correct."""
    from curdleproofs_pie_amd.prover_kernels import same_scalar_prove_device, same_scalar_prove_device_many

    N = native_lib
    k = Case(cases[3])                                                   # ell = 8
    ell, pb = k.ell, 576
    try:
        bad = P(O.g1_compress(torsion_point()))
        pr = k.prover()
        for where, pos in ((3, 5), (4, 0), (3, ell - 1)):                # in vec_R, in vec_S
            vec = list(pr[where])
            vec[pos] = bad
            bad_pr = pr[:where] + (vec,) + pr[where + 1:]
            t = k.transcript()
            start = state(t)
            with pytest.raises(N.NativeError, match=NOT_G1_TEXT):
                same_scalar_prove_device(k.table, *bad_pr, t)
            assert state(t) == start
            # in a batch: the whole call is refused, every transcript stays
            ts = [k.transcript(b"prover %d" % i) for i in range(3)]
            starts = [state(x) for x in ts]
            with pytest.raises(N.NativeError, match=NOT_G1_TEXT):
                same_scalar_prove_device_many(k.table, [k.prover(1), bad_pr, k.prover(2)], ts)
            assert [state(x) for x in ts] == starts
            t = k.transcript()                                           # the next valid call is correct
            assert to_bytes(same_scalar_prove_device(k.table, *pr, t)).hex() == k.raw["proof"]
            assert fr32(t.get_and_append_challenge(b"after")).hex() == k.raw["after"]
        # ---- the C entry: its own status, the output buffers as they were
        from curdleproofs_pie_amd.py_arkworks_bls12381 import points_to_affine96

        a = raw_args(k)
        a["rs"] = a["rs"][:96 * 2] + bytes(points_to_affine96([bad])) + a["rs"][96 * 3:]
        start = state(k.transcript())
        st = ctypes.create_string_buffer(start, 208)
        out = ctypes.create_string_buffer(b"\xaa" * pb, pb)
        assert call_raw(N, k.table._ctx.handle, k.table._tab.handle, ell, 1, a, st, out) == N.ERR_NOT_IN_SUBGROUP
        assert out.raw == b"\xaa" * pb and st.raw == start
        assert NOT_G1_TEXT in N.cg1_ctx_error(k.table._ctx.handle).decode()
    finally:
        k.table.close()


def test_refusals_leave_everything_untouched(native_lib, cases):
    from curdleproofs_pie_amd.prover_kernels import same_scalar_prove_device, same_scalar_prove_device_many

    N = native_lib
    k = Case(cases[2])                                                   # ell = 5
    ell, pb = k.ell, 576
    try:
        ctxh, tabh = k.table._ctx.handle, k.table._tab.handle
        start = state(k.transcript())

        def refused(want, ell_=ell, P_=1, tab_=tabh, **edit):
            a = raw_args(k, P_)
            a.update(edit)
            st = ctypes.create_string_buffer(start * P_, 208 * P_)
            out = ctypes.create_string_buffer(b"\xaa" * (pb * P_), pb * P_)
            rc = call_raw(N, ctxh, tab_, ell_, P_, a, st, out)
            assert (rc == want if want is not None else rc != N.OK), (edit.keys(), rc)
            assert out.raw == b"\xaa" * (pb * P_) and st.raw == start * P_

        def good(certified=0):
            a = raw_args(k)
            a["certified"] = certified
            st = ctypes.create_string_buffer(start, 208)
            out = ctypes.create_string_buffer(pb)
            assert call_raw(N, ctxh, tabh, ell, 1, a, st, out) == N.OK
            assert out.raw.hex() == k.raw["proof"] and st.raw != start

        good()
        good(certified=1)
        refused(N.ERR_ARG, ell_=0)
        refused(N.ERR_ARG, ell_=N.SAME_SCALAR_MAX_ELL + 1)
        refused(N.ERR_ARG, P_=N.SAME_SCALAR_MAX_PROVERS + 1)
        refused(N.ERR_ARG, tab_=None)
        for key in ("gth", "rs", "a", "k", "bl"):
            refused(N.ERR_ARG, **{key: None})
        a1024 = raw_args(k)                                              # 3 + 9 x 2 x 1024 bases: more than a light table holds
        refused(N.ERR_ARG, ell_=1024, P_=9, rs=bytes(96 * 2 * 1024 * 9), a=bytes(32 * 1024 * 9), k=a1024["k"] * 9, bl=a1024["bl"] * 9)
        good()
        for key in ("a", "k", "bl"):
            for bad in (R, (1 << 256) - 1):
                buf = bytearray(raw_args(k)[key])
                buf[-32:] = bad.to_bytes(32, "little")
                refused(N.ERR_ENCODING, **{key: bytes(buf)})
        buf = bytearray(raw_args(k)["bl"])                               # r_t, the first blinder
        buf[:32] = R.to_bytes(32, "little")
        refused(N.ERR_ENCODING, bl=bytes(buf))
        good()
        rs, gth = raw_args(k)["rs"], raw_args(k)["gth"]
        refused(None, rs=rs[:96 * 3] + O.P.to_bytes(48, "little") + rs[96 * 3 + 48:])            # an R coordinate >= p
        refused(None, rs=rs[:96 * 3] + b"\xff" * 48 + rs[96 * 3 + 48:])
        refused(N.ERR_NOT_ON_CURVE, rs=rs[:96 * (ell + 2)] + rs[96 * (ell + 3): 96 * (ell + 3) + 48] + rs[96 * (ell + 2) + 48:])   # S_2 with S_3's x
        assert "prover 0: entry %d of vec_R | vec_S" % (ell + 2) in N.cg1_ctx_error(ctxh).decode()
        refused(N.ERR_NOT_ON_CURVE, gth=gth[:96 * 2] + gth[:48] + gth[96 * 2 + 48:])              # H with G_t's x
        assert "crs_H" in N.cg1_ctx_error(ctxh).decode()
        refused(N.ERR_NOT_ON_CURVE, P_=3, rs=rs * 2 + rs[:96] + rs[96 * 2: 96 * 2 + 48] + rs[96 + 48:])      # prover 2, entry 1
        assert "prover 2: entry 1 of vec_R | vec_S" in N.cg1_ctx_error(ctxh).decode()
        good()
        # ---- the Python face: refusals raise and leave the caller's transcript alone
        t = k.transcript()
        pr = k.prover()
        with pytest.raises(ValueError):
            same_scalar_prove_device(k.table, k.Gt, k.Gu, k.H, k.vR[:4], k.vS, k.a, *pr[6:], t)
        with pytest.raises(ValueError):
            same_scalar_prove_device(k.table, k.Gt, k.Gu, k.H, [], [], [], *pr[6:], t)
        with pytest.raises(TypeError):
            same_scalar_prove_device(k.table, k.Gt, k.Gu, k.H, k.vR[:-1] + [b"\x00" * 48], k.vS, k.a, *pr[6:], t)
        with pytest.raises(N.NativeError):
            same_scalar_prove_device(k.table, *pr[:5], k.a[:-1] + [R], *pr[6:], t)                         # a plain int >= r
        with pytest.raises(N.NativeError):
            same_scalar_prove_device(k.table, *pr[:6], R + 1, *pr[7:], t)
        with pytest.raises(ValueError):
            same_scalar_prove_device_many(k.table, [pr], [])
        assert state(t) == start
        assert to_bytes(same_scalar_prove_device(k.table, *pr, t)).hex() == k.raw["proof"]                 # the next valid call is correct
        assert fr32(t.get_and_append_challenge(b"after")).hex() == k.raw["after"]
        assert same_scalar_prove_device_many(k.table, [], []) == []
    finally:
        k.table.close()
    with pytest.raises(N.NativeError):
        same_scalar_prove_device(k.table, *k.prover(), k.transcript())                                     # the table is closed


def test_four_device_provers_share_one_table(native_lib, cases):
    """ipa | same-scalar | same-MSM | same-scalar (larger ell: the light-table scratch regrows) | same-permutation | same-scalar on ONE
    table handle -- one staging block, laid out afresh by every call, and one light-table scratch for same-MSM and same-scalar -- each
    giving its fixture's bytes and transcript state."""
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.prover_kernels import (ipa_prove_device, same_msm_prove_device, same_permutation_prove_device,
                                                     same_scalar_prove_device)

    vec = lambda c, key: [S(h) for h in c[key]]
    pts = lambda c, key: [P(h) for h in c[key]]
    ipa_c = next(c for c in golden("ipa_device_vectors.json") if c["n"] == 8 and c.get("form") == "explicit")
    smsm_c = next(c for c in golden("same_msm_device_vectors.json") if c["n"] == 8)
    sperm_c = next(c for c in golden("same_permutation_device_vectors.json") if c["ell"] + c["n_blinders"] == 8)
    ipa = (pts(ipa_c, "crs_G_vec"), pts(ipa_c, "crs_G_prime_vec"), P(ipa_c["crs_H"]), P(ipa_c["C"]), P(ipa_c["D"]), S(ipa_c["z"]),
           vec(ipa_c, "vec_c"), vec(ipa_c, "vec_d"), vec(ipa_c, "vec_r_c"), vec(ipa_c, "vec_r_d"))
    smsm = (pts(smsm_c, "crs_G_vec"), P(smsm_c["A"]), P(smsm_c["Z_t"]), P(smsm_c["Z_u"]), pts(smsm_c, "vec_T"), pts(smsm_c, "vec_U"),
            vec(smsm_c, "vec_x"), vec(smsm_c, "vec_r"))
    sperm = (pts(sperm_c, "crs_G_vec"), pts(sperm_c, "crs_H_vec"), P(sperm_c["crs_U"]), P(sperm_c["A"]), P(sperm_c["M"]), vec(sperm_c, "vec_a"),
             list(sperm_c["permutation"]), vec(sperm_c, "vec_a_blinders"), vec(sperm_c, "vec_m_blinders"), vec(sperm_c, "vec_c_blinders"),
             vec(sperm_c, "ipa_r"), vec(sperm_c, "ipa_z_head"))
    ss = {ell: Case(c, own_table=False) for c in cases for ell in [c["ell"]] if ell in (5, 8, 28)}
    table = FixedBaseTable(ipa[0] + ipa[1] + [ipa[2]] + smsm[0] + sperm[0] + sperm[1] + [sperm[2]])

    def flat(res):
        out = b""
        for f in res:
            if isinstance(f, tuple):
                out += flat(f)
            else:
                for v in f if isinstance(f, list) else [f]:
                    out += bytes(v.to_compressed_bytes()) if hasattr(v, "to_compressed_bytes") else fr32(v)
        return out

    def transcript(c):
        from curdleproofs_pie_amd.merlin import CurdleproofsTranscript

        t = CurdleproofsTranscript(c["label"].encode())
        t.append(c["prefix_label"].encode(), bytes.fromhex(c["prefix"]))
        return t

    def run(fn, c, prover, encode=flat):
        t = transcript(c)
        assert encode(fn(table, *prover, t)).hex() == c["proof"], fn.__name__
        assert fr32(t.get_and_append_challenge(b"after")).hex() == c["after"], fn.__name__

    try:
        run(ipa_prove_device, ipa_c, ipa)
        run(same_scalar_prove_device, ss[5].raw, ss[5].prover(), to_bytes)
        run(same_msm_prove_device, smsm_c, smsm)
        run(same_scalar_prove_device, ss[28].raw, ss[28].prover(), to_bytes)
        run(same_permutation_prove_device, sperm_c, sperm)
        run(same_scalar_prove_device, ss[8].raw, ss[8].prover(), to_bytes)
        run(same_msm_prove_device, smsm_c, smsm)
    finally:
        table.close()
