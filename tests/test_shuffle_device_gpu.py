"""prover_kernels.shuffle_prove_device / cg1_shuffle_prove_device (csrc/capi_shuffle.h, csrc/kernels_shuffle.h): a whole shuffle proof --
CurdleProofsProof.new -- proved in one native call.  Needs an MI355X.

Pinned to the reference's bytes: tests/golden/shuffle_device_vectors.json records shuffle_permute_and_commit_input and
CurdleProofsProof.new run unmodified, with every draw.  Provers in step must each get what they get alone; the package's own batch
verifier accepts M || proof; seeded edge inputs are compared with the three existing device provers composed in Python as
curdleproofs.py:63-149 writes it; every refusal is a status word that leaves the outputs alone; and the call shares one table handle
with the other device provers."""
import ctypes
import json
import os
import random
import sys
import types

import pytest

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu
R = O.R
INF = b"\xc0" + bytes(47)
NB = 4
DRAW_KEYS = ("vec_a_blinders", "vec_c_blinders", "ipa_r", "ipa_z_head", "r_t", "r_u", "r_a", "r_b", "r_k", "vec_r")


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


def comp(p):
    return bytes(p.to_compressed_bytes())


def golden(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))["cases"]


@pytest.fixture(scope="module")
def cases(native_lib):
    return golden("shuffle_device_vectors.json")


def commit(crs, table, vR, vS, perm, k, mbl):
    """shuffle_permute_and_commit_input (curdleproofs.py:301-321) with the caller's vec_m_blinders: -> vec_T, vec_U, M."""
    from curdleproofs_pie_amd import Scalar
    from curdleproofs_pie_amd.msm_accumulator import batch_mul_same_scalar

    both = batch_mul_same_scalar(list(vR) + list(vS), k)
    ell = len(vR)
    M = table.msm([Scalar(j) for j in perm] + list(mbl), list(crs.vec_G) + list(crs.vec_H))
    return [both[j] for j in perm], [both[ell + j] for j in perm], M


class Case:
    """A fixture case as product objects, over a FixedBaseTable of vec_G | vec_H | H | G_t | G_u."""

    def __init__(self, case, decode=P, extra_bases=()):
        from curdleproofs_pie_amd.fixed_base import FixedBaseTable

        self.raw, self.ell = case, case["ell"]
        ell, n = self.ell, self.ell + NB
        if "vec_G" in case:
            enc = case["vec_G"] + case["vec_H"] + [case["H"], case["G_t"], case["G_u"]] + case["vec_R"] + case["vec_S"]
            pts = [decode(h) for h in enc]
        else:                                                            # not stored: G1 * k, the n + 3 + 2 ell scalars k the case's seed gives first
            from curdleproofs_pie_amd import G1Point, Scalar
            from curdleproofs_pie_amd.msm_accumulator import batch_mul

            rng = random.Random(case["seed"])
            count = n + 3 + 2 * ell
            pts = batch_mul([G1Point()] * count, [Scalar(rng.randint(1, R - 1)) for _ in range(count)])
            pts = [decode(comp(p)) for p in pts]
        self.crs = types.SimpleNamespace(vec_G=pts[:ell], vec_H=pts[ell:n], H=pts[n], G_t=pts[n + 1], G_u=pts[n + 2])
        self.vR, self.vS = pts[n + 3: n + 3 + ell], pts[n + 3 + ell:]
        self.vT, self.vU = [decode(h) for h in case["vec_T"]], [decode(h) for h in case["vec_U"]]
        self.M, self.perm, self.k = P(case["M"]), list(case["permutation"]), S(case["k"])
        self.mbl = [S(h) for h in case["vec_m_blinders"]]
        d = case["draws"]
        self.draws = tuple([S(h) for h in d[key]] if isinstance(d[key], list) else S(d[key]) for key in DRAW_KEYS)
        self.table = FixedBaseTable(pts[:n + 3] + list(extra_bases))
        self._provers = {}

    def prover(self, rot=0):
        """Prover `rot` of a call in step: prover 0 is the fixture's; the others have rotated vec_R and vec_S (S reversed for odd rot),
        their own k, permutation, vec_m_blinders and draws, and the vec_T, vec_U and M that go with them."""
        from curdleproofs_pie_amd import Scalar

        if rot in self._provers:
            return self._provers[rot]
        if rot == 0:
            pr = (self.crs, self.vR, self.vS, self.vT, self.vU, self.M, self.perm, self.k, self.mbl, self.draws)
        else:
            r = lambda v, j: v[j % len(v):] + v[:j % len(v)]
            vR, vS = r(self.vR, rot), r(self.vS, 2 * rot)
            if rot % 2:
                vS = vS[::-1]
            perm = list(range(self.ell))
            random.Random(1000 * self.ell + rot).shuffle(perm)
            k = self.k + Scalar(rot)
            mbl = [b + Scalar(3 * rot + i) for i, b in enumerate(self.mbl)]
            bump = iter(range(1, 1 << 20))
            draws = tuple([s + Scalar(rot * next(bump)) for s in d] if isinstance(d, list) else d + Scalar(rot * next(bump)) for d in self.draws)
            vT, vU, M = commit(self.crs, self.table, vR, vS, perm, k, mbl)
            pr = (self.crs, vR, vS, vT, vU, M, perm, k, mbl, draws)
        self._provers[rot] = pr
        return pr


def flat(res):
    out = b""
    for f in res:
        if isinstance(f, tuple):
            out += flat(f)
        else:
            for v in f if isinstance(f, list) else [f]:
                out += comp(v) if hasattr(v, "to_compressed_bytes") else fr32(v)
    return out


def composed(table, crs, vR, vS, vT, vU, M, perm, k, mbl, draws):
    """The parent's best path: curdleproofs.py:63-149 written out in Python over compute_MSM for A and the three existing device provers."""
    from curdleproofs_pie_amd import G1Point, Scalar
    from curdleproofs_pie_amd.merlin import CurdleproofsTranscript
    from curdleproofs_pie_amd.msm_accumulator import compute_MSM
    from curdleproofs_pie_amd.prover_kernels import same_msm_prove_device, same_permutation_prove_device, same_scalar_prove_device

    ell = len(vR)
    abl, cbl, ipa_r, z_head, r_t, r_u, r_a, r_b, r_k, vec_r = draws
    t = CurdleproofsTranscript(b"curdleproofs")
    t.append_list(b"curdleproofs_step1", [comp(p) for p in list(vR) + list(vS) + list(vT) + list(vU)])
    t.append(b"curdleproofs_step1", comp(M))
    vec_a = t.get_and_append_challenges(b"curdleproofs_vec_a", ell)
    abl4 = list(abl) + [Scalar(0), Scalar(0)]
    a_perm = [vec_a[j] for j in perm]
    A = compute_MSM(list(crs.vec_G) + list(crs.vec_H), a_perm + abl4)
    sp = same_permutation_prove_device(table, crs.vec_G, crs.vec_H, crs.H, A, M, vec_a, list(perm), abl4, list(mbl), list(cbl), list(ipa_r), list(z_head), t)
    R_, S_, cm_T, cm_U, cm_A, cm_B, z_k, z_t, z_u = same_scalar_prove_device(table, crs.G_t, crs.G_u, crs.H, vR, vS, vec_a, k, r_t, r_u, r_a, r_b, r_k, t)
    A_prime = A + cm_T[0] + cm_U[0]
    Z1 = G1Point.identity()
    sm = same_msm_prove_device(table, list(crs.vec_G) + list(crs.vec_H[:2]) + [crs.G_t, crs.G_u], A_prime, cm_T[1], cm_U[1], list(vT) + [Z1, Z1, crs.H, Z1],
                               list(vU) + [Z1, Z1, Z1, crs.H], a_perm + list(abl) + [r_t, r_u], list(vec_r), t)
    return comp(A) + flat((cm_T, cm_U, R_, S_)) + flat(sp) + flat((cm_A, cm_B, z_k, z_t, z_u)) + flat(sm)


def snapshot(pr):
    """Everything a prover tuple holds, as bytes: to see that a call mutated nothing."""
    crs, vR, vS, vT, vU, M, perm, k, mbl, draws = pr
    return (flat((list(vR), list(vS), list(vT), list(vU), M, k, list(mbl), tuple(draws))), list(perm), [x._sg for x in list(vR) + list(vS)])


@pytest.mark.parametrize("certified", [False, True])
@pytest.mark.parametrize("which", range(4))
def test_fixture_cases_reproduce_reference_bytes(native_lib, cases, which, certified):
    """ell = 4, 12, 28, 124, with the subgroup launch (bases decoded unchecked) and without it (bases that carry their certificate)."""
    from curdleproofs_pie_amd.prover_kernels import shuffle_prove_device

    k = Case(cases[which], decode=Pc if certified else P)
    try:
        assert all((x._sg is True) == certified for x in k.vR + k.vS)
        before = snapshot(k.prover())
        for _ in range(2):
            raw = shuffle_prove_device(k.table, *k.prover())
            assert len(raw) == native_lib.cg1_shuffle_prover_proof_bytes(k.ell)
            assert raw.hex() == k.raw["proof"], k.ell
        assert snapshot(k.prover()) == before
    finally:
        k.table.close()


@pytest.mark.parametrize("which,batches", [(0, (64,)), (1, (1, 3, 8)), (2, (1, 3, 8))])
def test_provers_in_step(cases, which, batches):
    """Batches of 1, 3 and 8 at ell = 12 and 28, and 64 at ell = 4: every prover's bytes equal what it gets alone, all distinct."""
    from curdleproofs_pie_amd.prover_kernels import shuffle_prove_device_many

    k = Case(cases[which])
    try:
        alone = {}
        for batch in batches:
            provers = [k.prover(i) for i in range(batch)]
            got = shuffle_prove_device_many(k.table, provers)
            assert len(got) == batch and got[0].hex() == k.raw["proof"]
            for i in range(1, batch):
                if i not in alone:
                    alone[i] = shuffle_prove_device_many(k.table, [provers[i]])[0]
                assert got[i] == alone[i], (batch, i)
            assert len(set(got)) == batch
    finally:
        k.table.close()


def test_more_provers_than_one_call_carries(cases):
    """70 provers at ell = 4: calls of 64 and 6.  A sample, first and last included, equals what each gets alone."""
    from curdleproofs_pie_amd.prover_kernels import shuffle_prove_device_many

    k = Case(cases[0])
    try:
        provers = [k.prover(i) for i in range(70)]
        got = shuffle_prove_device_many(k.table, provers)
        assert len(got) == 70 and got[0].hex() == k.raw["proof"]
        for i in (0, 1, 63, 64, 69):
            assert got[i] == shuffle_prove_device_many(k.table, [provers[i]])[0], i
    finally:
        k.table.close()


def crs_bytes(crs):
    from functools import reduce
    return b"".join(comp(p) for p in list(crs.vec_G) + list(crs.vec_H) + [crs.H, crs.G_t, crs.G_u, reduce(lambda a, b: a + b, crs.vec_G), reduce(lambda a, b: a + b, crs.vec_H)])


def test_the_batch_verifier_accepts(native_lib, cases):
    """M || proof for a batch of 8 at ell = 28 is accepted by are_valid_whisk_shuffle_proofs over the same CRS; a flipped byte in z_k is not."""
    from curdleproofs_pie_amd.prover_kernels import shuffle_prove_device_many
    from curdleproofs_pie_amd.shuffle_verifier import are_valid_whisk_shuffle_proofs

    N = native_lib
    k = Case(cases[2])
    try:
        provers = [k.prover(i) for i in range(8)]
        got = shuffle_prove_device_many(k.table, provers)
        items = []
        for pr, raw in zip(provers, got):
            _, vR, vS, vT, vU, M = pr[:6]
            items.append(([(comp(r), comp(s)) for r, s in zip(vR, vS)], [(comp(t), comp(u)) for t, u in zip(vT, vU)], comp(M) + raw))
        crs = crs_bytes(k.crs)
        assert are_valid_whisk_shuffle_proofs(crs, items) == [True] * 8
        z_k = 48 + 336 + N.cg1_same_perm_proof_bytes(k.ell, NB) + 192
        pre, post, proof = items[3]
        bad = proof[:z_k + 5] + bytes([proof[z_k + 5] ^ 1]) + proof[z_k + 6:]
        assert are_valid_whisk_shuffle_proofs(crs, items[:3] + [(pre, post, bad)] + items[4:]) == [True] * 3 + [False] + [True] * 4
    finally:
        k.table.close()


def test_edge_inputs_against_the_composed_path(cases):
    """Seeded inputs without a fixture, at ell = 4 over the first case's CRS: the whole-shuffle call and the parent's path -- compute_MSM
    for A, then the three device provers composed in Python -- give the same bytes."""
    from curdleproofs_pie_amd import Scalar
    from curdleproofs_pie_amd.prover_kernels import shuffle_prove_device

    k = Case(cases[0])
    ell = k.ell
    rng = random.Random(9101)
    rpt = lambda: P(O.g1_compress(O.g1_mul(O.G1_GEN, rng.randrange(1, R))))
    rs = lambda m: [Scalar(rng.randrange(1, R)) for _ in range(m)]
    draws = lambda: (rs(2), rs(NB), rs(ell + NB), rs(ell + NB - 2), *rs(5), rs(ell + NB))
    ident = P(INF)
    vR, vS = [rpt() for _ in range(ell)], [rpt() for _ in range(ell)]
    perm = [2, 0, 3, 1]
    zero_rt = list(draws())
    zero_rt[4] = Scalar(0)
    zero_abl = list(draws())
    zero_abl[0] = [Scalar(0), Scalar(0)]
    # name: (vec_R, vec_S, permutation, k, draws)
    shapes = {
        "identities in vec_R and vec_T": ([vR[0], ident, vR[2], ident], vS, perm, rs(1)[0], draws()),
        "k = 0": (vR, vS, perm, Scalar(0), draws()),
        "r_t = 0": (vR, vS, perm, rs(1)[0], tuple(zero_rt)),
        "vec_a_blinders zero": (vR, vS, perm, rs(1)[0], tuple(zero_abl)),
        "a permutation that is no bijection": (vR, vS, [1, 1, 3, 1], rs(1)[0], draws()),
        "repeated trackers": ([vR[0], vR[0], vR[1], vR[0]], [vS[0], vS[0], vS[1], vS[0]], perm, rs(1)[0], draws()),
    }
    try:
        for name, (R_, S_, pm, kk, dr) in shapes.items():
            mbl = rs(NB)
            vT, vU, M = commit(k.crs, k.table, R_, S_, pm, kk, mbl)
            pr = (k.crs, R_, S_, vT, vU, M, pm, kk, mbl, dr)
            got = shuffle_prove_device(k.table, *pr)
            assert got == composed(k.table, *pr), name
            if name == "k = 0":
                assert all(comp(p) == INF for p in vT + vU)
            if name == "r_t = 0":
                assert got[48:96] == INF                                 # cm_T.T_1 = r_t G_t
            if name.startswith("identities"):
                assert comp(vT[2]) == comp(vT[3]) == INF and comp(vT[1]) != INF      # perm[2] = 3 and perm[3] = 1 -> O; perm[1] = 0 -> R_0 k
    finally:
        k.table.close()


def raw_args(k, P_=1):
    """The C entry's arguments for P_ copies of a fixture case."""
    from curdleproofs_pie_amd.py_arkworks_bls12381 import points_to_affine96

    ell, t, crs = k.ell, k.table, k.crs
    vec = lambda *keys: b"".join(b"".join(bytes.fromhex(h) for h in k.raw["draws"][key]) if isinstance(k.raw["draws"][key], list) else bytes.fromhex(k.raw["draws"][key])
                                 for key in keys) * P_
    return dict(gi=list(t._indices(crs.vec_G, ell)) * P_, hi=list(t._indices(crs.vec_H, NB)) * P_, ui=[t.index(crs.H)] * P_, gti=[t.index(crs.G_t)] * P_,
                gui=[t.index(crs.G_u)] * P_, gth=bytes(points_to_affine96([crs.G_t, crs.G_u, crs.H])), rs=bytes(points_to_affine96(k.vR + k.vS)) * P_,
                tu=bytes(points_to_affine96(k.vT + k.vU)) * P_, m=bytes.fromhex(k.raw["M"]) * P_, perm=list(k.perm) * P_, k=bytes.fromhex(k.raw["k"]) * P_,
                mbl=b"".join(bytes.fromhex(h) for h in k.raw["vec_m_blinders"]) * P_, abl=vec("vec_a_blinders"), cbl=vec("vec_c_blinders"), r=vec("ipa_r"),
                z=vec("ipa_z_head"), bl=vec("r_t", "r_u", "r_a", "r_b", "r_k"), vr=vec("vec_r"), certified=0)


def call_raw(N, ctx_handle, tab_handle, ell, P_, a, out):
    u32 = lambda v: None if v is None else (ctypes.c_uint32 * max(1, len(v)))(*v)
    return N.cg1_shuffle_prove_device(ctx_handle, tab_handle, ell, P_, u32(a["gi"]), u32(a["hi"]), u32(a["ui"]), u32(a["gti"]), u32(a["gui"]), a["gth"], a["rs"], a["tu"],
                                      a["m"], u32(a["perm"]), a["k"], a["mbl"], a["abl"], a["cbl"], a["r"], a["z"], a["bl"], a["vr"], a["certified"], out, None)


def torsion_point():
    """T3 + P for the order-3 point T3 of tests/golden/torsion_vectors.json: on the curve, of order 3 r, outside G1."""
    tors = json.load(open(os.path.join(ROOT, "tests", "golden", "torsion_vectors.json")))
    T3 = O.g1_decompress(bytes.fromhex(tors["t3"]))
    assert not O.g1_in_subgroup(T3) and O.g1_mul(T3, 3) is None
    pt = O.g1_add(T3, O.g1_mul(O.G1_GEN, 0x5EED))
    assert not O.g1_in_subgroup(pt)
    return pt


def test_refusals_leave_everything_untouched(native_lib, cases):
    from curdleproofs_pie_amd import Scalar
    from curdleproofs_pie_amd.prover_kernels import shuffle_prove_device, shuffle_prove_device_many
    from curdleproofs_pie_amd.py_arkworks_bls12381 import points_to_affine96

    N = native_lib
    k = Case(cases[1])                                                   # ell = 12
    ell, n = k.ell, k.ell + NB
    pb = N.cg1_shuffle_prover_proof_bytes(ell)
    who = "cg1_shuffle_prove_device"
    try:
        ctxh, tabh = k.table._ctx.handle, k.table._tab.handle

        def refused(want, text=None, ell_=ell, P_=1, tab_=tabh, **edit):
            a = raw_args(k, P_)
            a.update(edit)
            out = ctypes.create_string_buffer(b"\xaa" * (pb * P_), pb * P_)
            rc = call_raw(N, ctxh, tab_, ell_, P_, a, out)
            assert (rc == want if want is not None else rc != N.OK), (edit.keys(), rc)
            assert out.raw == b"\xaa" * (pb * P_)
            err = N.cg1_ctx_error(ctxh).decode()
            assert err.startswith(who) and (text is None or text in err), err

        def good():
            out = ctypes.create_string_buffer(pb)
            assert call_raw(N, ctxh, tabh, ell, 1, raw_args(k), out) == N.OK
            assert out.raw.hex() == k.raw["proof"]

        good()
        refused(N.ERR_ARG, "power of two", ell_=5)                      # ell = 5: n = 9
        refused(N.ERR_ARG, "provers", P_=65)
        for key in ("gi", "hi", "ui", "gti", "gui", "gth", "rs", "tu", "m", "perm", "k", "mbl", "abl", "cbl", "r", "z", "bl", "vr"):
            refused(N.ERR_ARG, "bad argument", **{key: None})
        refused(N.ERR_ARG, "bad argument", tab_=None)
        good()
        for key in ("k", "mbl", "abl", "cbl", "r", "z", "bl", "vr"):   # a scalar >= r in each scalar array
            for bad in (R, (1 << 256) - 1):
                buf = bytearray(raw_args(k)[key])
                buf[-32:] = bad.to_bytes(32, "little")
                refused(N.ERR_ENCODING, ">= r", **{key: bytes(buf)})
        refused(N.ERR_ARG, "permutation entry", perm=k.perm[:-1] + [ell])
        refused(N.ERR_ARG, "outside the table", gi=[len(k.table)] + raw_args(k)["gi"][1:])
        good()
        tu = raw_args(k)["tu"]
        refused(N.ERR_NOT_ON_CURVE, "vec_T | vec_U", tu=tu[:96 * 2] + tu[96 * 3: 96 * 3 + 48] + tu[96 * 2 + 48:])       # T_2 with T_3's x
        rs = raw_args(k)["rs"]
        refused(N.ERR_NOT_IN_SUBGROUP, "outside the prime-order subgroup", rs=rs[:96 * 2] + bytes(points_to_affine96([P(O.g1_compress(torsion_point()))])) + rs[96 * 3:])
        good()
        # ---- the Python face
        pr = k.prover()
        before = snapshot(pr)
        wrong_M = P(O.g1_compress(O.g1_mul(O.G1_GEN, 77)))
        with pytest.raises(N.NativeError, match="M is not the commitment"):
            shuffle_prove_device(k.table, *pr[:5], wrong_M, *pr[6:])
        with pytest.raises(ValueError):
            shuffle_prove_device(k.table, k.crs, k.vR[:5], k.vS[:5], k.vT[:5], k.vU[:5], k.M, k.perm[:5], k.k, k.mbl, k.draws)      # ell = 5
        with pytest.raises(ValueError):
            shuffle_prove_device(k.table, *pr[:3], k.vT[:-1], *pr[4:])
        with pytest.raises(ValueError):
            shuffle_prove_device(k.table, *pr[:9], k.draws[:-1])
        with pytest.raises(ValueError):
            shuffle_prove_device(k.table, *pr[:6], k.perm[:-1] + [-1], *pr[7:])
        with pytest.raises(TypeError):
            shuffle_prove_device(k.table, *pr[:1], k.vR[:-1] + [b"\x00" * 48], *pr[2:])
        with pytest.raises(TypeError):
            shuffle_prove_device(k.table, *pr[:7], 5, *pr[8:])                                               # k as a plain int
        with pytest.raises(N.NativeError):
            shuffle_prove_device(k.table, *pr[:7], Scalar._raw(R), *pr[8:])
        assert snapshot(pr) == before
        assert shuffle_prove_device(k.table, *pr).hex() == k.raw["proof"]                                    # the next valid call is correct
        assert shuffle_prove_device_many(k.table, []) == []
    finally:
        k.table.close()
    with pytest.raises(N.NativeError):
        shuffle_prove_device(k.table, *k.prover())                                                           # the table is closed


def test_one_table_handle_shared(native_lib, cases):
    """ipa | whole shuffle | same-MSM on ONE table handle -- one staging block, laid out afresh by every call, one light-table scratch --
    each giving its fixture's bytes."""
    from curdleproofs_pie_amd.merlin import CurdleproofsTranscript
    from curdleproofs_pie_amd.prover_kernels import ipa_prove_device, same_msm_prove_device, shuffle_prove_device

    vec = lambda c, key: [S(h) for h in c[key]]
    pts = lambda c, key: [P(h) for h in c[key]]
    ipa_c = next(c for c in golden("ipa_device_vectors.json") if c["n"] == 8 and c.get("form") == "explicit")
    smsm_c = next(c for c in golden("same_msm_device_vectors.json") if c["n"] == 8)
    ipa = (pts(ipa_c, "crs_G_vec"), pts(ipa_c, "crs_G_prime_vec"), P(ipa_c["crs_H"]), P(ipa_c["C"]), P(ipa_c["D"]), S(ipa_c["z"]),
           vec(ipa_c, "vec_c"), vec(ipa_c, "vec_d"), vec(ipa_c, "vec_r_c"), vec(ipa_c, "vec_r_d"))
    smsm = (pts(smsm_c, "crs_G_vec"), P(smsm_c["A"]), P(smsm_c["Z_t"]), P(smsm_c["Z_u"]), pts(smsm_c, "vec_T"), pts(smsm_c, "vec_U"),
            vec(smsm_c, "vec_x"), vec(smsm_c, "vec_r"))
    k = Case(cases[1], extra_bases=ipa[0] + ipa[1] + [ipa[2]] + smsm[0])

    def run(fn, c, prover):
        t = CurdleproofsTranscript(c["label"].encode())
        t.append(c["prefix_label"].encode(), bytes.fromhex(c["prefix"]))
        assert flat(fn(k.table, *prover, t)).hex() == c["proof"], fn.__name__
        assert fr32(t.get_and_append_challenge(b"after")).hex() == c["after"], fn.__name__

    try:
        run(ipa_prove_device, ipa_c, ipa)
        assert shuffle_prove_device(k.table, *k.prover()).hex() == k.raw["proof"]
        run(same_msm_prove_device, smsm_c, smsm)
        assert shuffle_prove_device(k.table, *k.prover()).hex() == k.raw["proof"]
    finally:
        k.table.close()
