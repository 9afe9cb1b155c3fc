"""prover_kernels.same_permutation_prove_device / cg1_same_perm_prove_device (csrc/kernels_same_perm.h, then k_gprod_step's step phase and
the phases of csrc/kernels_ipa.h): the whole same-permutation argument as the grand-product launch chain with another head.  Needs an MI355X.

Pinned to the reference's bytes: tests/golden/same_permutation_device_vectors.json records SamePermutationProof.new run stand-alone (proof
bytes, and a challenge drawn after it that pins the final transcript state).  Provers in step must each get what they get alone; edge
inputs are compared with a host-driven path written here (Python ints, the host transcript, B from table.msm, then the merged
grand_product_prove_device); every refusal leaves the outputs and the transcript alone; and same-permutation calls between inner-product,
same-MSM and grand-product calls on one table handle share their staging block."""
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


def P(h):
    from curdleproofs_pie_amd.py_arkworks_bls12381 import G1Point
    return G1Point.from_compressed_bytes_unchecked(bytes.fromhex(h))


def S(h):
    from curdleproofs_pie_amd.py_arkworks_bls12381 import Scalar
    return Scalar.from_le_bytes(bytes.fromhex(h))


def fr32(s):
    return bytes(s.to_le_bytes())


def golden_raw(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))


def golden(name):
    return golden_raw(name)["cases"]


@pytest.fixture(scope="module")
def cases(native_lib):
    return golden("same_permutation_device_vectors.json")


class Case:
    """A fixture case as product objects, with its table: crs_G_vec | crs_H_vec | crs_U."""

    def __init__(self, case, own_table=True):
        from curdleproofs_pie_amd.fixed_base import FixedBaseTable

        self.raw, self.ell, self.nb = case, case["ell"], case["n_blinders"]
        self.n = self.ell + self.nb
        if "crs_G_vec" in case:
            self.G, self.H, self.U = [P(h) for h in case["crs_G_vec"]], [P(h) for h in case["crs_H_vec"]], P(case["crs_U"])
        else:                                                            # not stored: G1 * k, the n + 1 scalars k the case's seed gives first
            from curdleproofs_pie_amd import G1Point, Scalar
            from curdleproofs_pie_amd.msm_accumulator import batch_mul

            rng = random.Random(case["seed"])
            pts = batch_mul([G1Point()] * (self.n + 1), [Scalar(rng.randint(1, R - 1)) for _ in range(self.n + 1)])
            self.G, self.H, self.U = pts[:self.ell], pts[self.ell:self.n], pts[self.n]
        self.table = FixedBaseTable(self.G + self.H + [self.U]) if own_table else None      # else: the caller's, over these objects
        self.A, self.M, self.perm = P(case["A"]), P(case["M"]), list(case["permutation"])
        vec = lambda key: [S(h) for h in case[key]]
        self.a, self.abl, self.mbl = vec("vec_a"), vec("vec_a_blinders"), vec("vec_m_blinders")
        self.cbl, self.r, self.zh = vec("vec_c_blinders"), vec("ipa_r"), vec("ipa_z_head")

    def transcript(self, prefix=None):
        from curdleproofs_pie_amd.merlin import CurdleproofsTranscript

        t = CurdleproofsTranscript(self.raw["label"].encode())
        t.append(self.raw["prefix_label"].encode(), bytes.fromhex(self.raw["prefix"]) if prefix is None else prefix)
        return t

    def prover(self, rot=0):
        """Prover `rot` of a call in step: rotated vectors, a rotated permutation and one changed a, so A and M are its own (recomputed here)."""
        from curdleproofs_pie_amd import Scalar

        if rot == 0:
            return (self.G, self.H, self.U, self.A, self.M, self.a, self.perm, self.abl, self.mbl, self.cbl, self.r, self.zh)
        r = lambda v, k: v[k % len(v):] + v[:k % len(v)]
        a = r(self.a, rot)
        a[0] = a[0] + Scalar(rot)
        perm, abl, mbl = r(self.perm, rot), r(self.abl, rot), r(self.mbl, rot + 1)
        vec_G = list(self.G) + list(self.H)
        A = self.table.msm([a[m] for m in perm] + abl, vec_G)
        M = self.table.msm([Scalar(m) for m in perm] + mbl, vec_G)
        return (self.G, self.H, self.U, A, M, a, perm, abl, mbl, r(self.cbl, 2 * rot), r(self.r, 3 * rot), r(self.zh, rot))


def gprod_bytes(res):
    """GrandProductProof.to_bytes: C | r_p | IPA.to_bytes (B_c | B_d | vec_L_C | vec_R_C | vec_L_D | vec_R_D | c_final | d_final)."""
    C, r_p, (B_c, B_d, LC, RC, LD, RD, c_fin, d_fin) = res
    comp = lambda p: bytes(p.to_compressed_bytes())
    return comp(C) + fr32(r_p) + b"".join(comp(p) for p in [B_c, B_d] + LC + RC + LD + RD) + fr32(c_fin) + fr32(d_fin)


def to_bytes(res):
    """SamePermutationProof.to_bytes: B | GrandProductProof.to_bytes."""
    B, gp = res
    return bytes(B.to_compressed_bytes()) + gprod_bytes(gp)


def state(t):
    return bytes(t.strobe._st.raw)


def host_driven(table, G, H, U, A, M, a, perm, abl, mbl, cbl, r, zh, transcript):
    """SamePermutationProof.new after its callee's draws with the wrapper driven from the host: the host transcript, the factors and their
    product in Python ints, B as one table.msm, then the grand-product argument's device chain."""
    from curdleproofs_pie_amd import G1Point, Scalar
    from curdleproofs_pie_amd.prover_kernels import grand_product_prove_device

    comp = lambda p: bytes(p.to_compressed_bytes()) if type(p) is G1Point else bytes(p)
    transcript.append_list(b"same_perm_step1", [comp(A), comp(M)])
    transcript.append_list(b"same_perm_step1", [fr32(x) for x in a])
    alpha = int(transcript.get_and_append_challenge(b"same_perm_alpha"))
    beta = int(transcript.get_and_append_challenge(b"same_perm_beta"))
    ai = [int(x) for x in a]
    b = [(ai[m] + m * alpha + beta) % R for m in perm]
    prod = 1
    for x in b:
        prod = prod * x % R
    bbl = [(int(x) + alpha * int(y)) % R for x, y in zip(abl, mbl)]
    sc = lambda v: [Scalar(x) for x in v]
    B = table.msm(sc(b + bbl), list(G) + list(H))
    return (B, grand_product_prove_device(table, G, H, U, B, Scalar(prod), sc(b), sc(bbl), cbl, r, zh, transcript))


@pytest.fixture(scope="module")
def big(cases):
    """The (508, 4) case with its table of 513 bases: shared with the ell = 300 edge input."""
    k = Case(cases[6])
    yield k
    k.table.close()


@pytest.mark.parametrize("which", range(7))
def test_fixture_cases_reproduce_reference_bytes(cases, big, which):
    from curdleproofs_pie_amd.prover_kernels import same_permutation_prove_device

    k = big if which == 6 else Case(cases[which])
    try:
        for _ in range(2):                                               # again: the same bytes, the same state
            t = k.transcript()
            res = same_permutation_prove_device(k.table, *k.prover(), t)
            assert to_bytes(res).hex() == k.raw["proof"], (k.ell, k.nb)
            assert state(t) != state(k.transcript())
            assert fr32(t.get_and_append_challenge(b"after")).hex() == k.raw["after"]
    finally:
        if k is not big:
            k.table.close()


@pytest.mark.parametrize("which", [3, 4])
def test_provers_in_step(cases, which):
    """Batches of 1, 3, 8 and 64 provers at (4, 4) and (28, 4): rotated vectors, permutations and blinders, their own A and M, different
    transcript prefixes; prover 0 is the fixture's; every prover's bytes and final state equal what it gets alone."""
    from curdleproofs_pie_amd.prover_kernels import same_permutation_prove_device_many

    k = Case(cases[which])
    assert (k.ell, k.nb) in ((4, 4), (28, 4))
    try:
        alone = {}
        all_provers = [k.prover(rot=i) for i in range(64)]
        for batch in (1, 3, 8, 64):
            provers = all_provers[:batch]
            prefix = lambda i: None if i == 0 else b"prover %d" % i
            ts = [k.transcript(prefix(i)) for i in range(batch)]
            got = same_permutation_prove_device_many(k.table, provers, ts)
            assert len(got) == batch
            assert to_bytes(got[0]).hex() == k.raw["proof"] and fr32(ts[0].get_and_append_challenge(b"after")).hex() == k.raw["after"]
            for i in range(1, batch):
                if i not in alone:
                    t1 = k.transcript(prefix(i))
                    alone[i] = (to_bytes(same_permutation_prove_device_many(k.table, [provers[i]], [t1])[0]), state(t1))
                assert (to_bytes(got[i]), state(ts[i])) == alone[i], (batch, i)
            assert len({to_bytes(g) for g in got}) == batch
    finally:
        k.table.close()


def test_edge_inputs_against_the_host_driven_path(native_lib, big):
    """Seeded random inputs: a permutation that is no bijection (repeated and missing indices), repeated base indices, a base outside G1,
    and ell = 300 (n = 512: a second scan shape, 212 blinders) over the big table -- the device chain and the host-driven path give the
    same bytes and the same transcript."""
    from curdleproofs_pie_amd import G1Point, Scalar
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.merlin import CurdleproofsTranscript
    from curdleproofs_pie_amd.prover_kernels import same_permutation_prove_device

    rng = random.Random(7201)
    tors = golden_raw("torsion_vectors.json")
    T3 = O.g1_decompress(bytes.fromhex(tors["t3"]))
    assert not O.g1_in_subgroup(T3)
    n = 16
    pts = [O.g1_mul(O.G1_GEN, rng.randrange(1, R)) for _ in range(n + 1)]
    pts[5] = O.g1_add(T3, pts[5])                                        # order 3 r: outside G1
    objs = [G1Point.from_compressed_bytes_unchecked(O.g1_compress(p)) for p in pts]
    tab = FixedBaseTable(objs)
    rs = lambda m: [Scalar(rng.randrange(1, R)) for _ in range(m)]
    shuffled = lambda m: rng.sample(range(m), m)
    shapes = {
        "no bijection": (tab, list(range(12)), list(range(12, 16)), n, [3, 3, 0, 11, 7, 3, 0, 9, 9, 9, 1, 11]),
        "repeated bases": (tab, [3] * 12, [13, 13, 14, 3], 3, shuffled(12)),
        "outside G1": (tab, list(range(14)), [14, 15], n, shuffled(14)),                        # index 5 is among crs_G_vec
        "ell 300": (big.table, list(range(300)), list(range(300, 512)), 512, shuffled(300)),
    }
    try:
        for name, (table, gi, hi, ui, perm) in shapes.items():
            ell, nb = len(gi), len(hi)
            m = ell + nb
            a, abl, mbl, cbl, r, zh = rs(ell), rs(nb), rs(nb), rs(nb), rs(m), rs(m - 2)
            A = table.msm([a[j] for j in perm] + abl, gi + hi)
            M = table.msm([Scalar(j) for j in perm] + mbl, gi + hi)
            mk = lambda: CurdleproofsTranscript(b"edge " + name.encode())
            t_dev, t_host = mk(), mk()
            keep = [list(v) for v in (a, perm, abl, mbl, cbl, r, zh)]
            got = same_permutation_prove_device(table, gi, hi, ui, A, M, a, perm, abl, mbl, cbl, r, zh, t_dev)
            assert [list(v) for v in (a, perm, abl, mbl, cbl, r, zh)] == keep, name            # no input is mutated
            want = host_driven(table, gi, hi, ui, A, M, a, perm, abl, mbl, cbl, r, zh, t_host)
            assert to_bytes(got) == to_bytes(want), name
            assert state(t_dev) == state(t_host), name
    finally:
        tab.close()


def raw_args(k, P=1):
    """The C entry's arguments for P copies of a fixture case."""
    n = k.n
    vec = lambda *keys: b"".join(bytes.fromhex(h) for key in keys for h in k.raw[key]) * P
    return dict(gi=(ctypes.c_uint32 * (n * P))(*(list(range(n)) * P)), ui=(ctypes.c_uint32 * P)(*([n] * P)), am=bytes.fromhex(k.raw["A"] + k.raw["M"]) * P,
                a=vec("vec_a"), perm=(ctypes.c_uint32 * (k.ell * P))(*(k.perm * P)), abl=vec("vec_a_blinders"), mbl=vec("vec_m_blinders"),
                cbl=vec("vec_c_blinders"), r=vec("ipa_r"), zh=vec("ipa_z_head"))


def call_raw(N, ctx_handle, tab_handle, ell, nb, P, a, st, out):
    return N.cg1_same_perm_prove_device(ctx_handle, tab_handle, ell, nb, P, a["gi"], a["ui"], a["am"], a["a"], a["perm"], a["abl"], a["mbl"], a["cbl"], a["r"], a["zh"],
                                        st, out, None)


def test_refusals_leave_everything_untouched(native_lib, cases):
    from curdleproofs_pie_amd import Scalar
    from curdleproofs_pie_amd.prover_kernels import same_permutation_prove_device, same_permutation_prove_device_many

    N = native_lib
    k = Case(cases[3])                                                    # (4, 4)
    n, pb = k.n, 864
    try:
        ctxh, tabh = k.table._ctx.handle, k.table._tab.handle
        start = state(k.transcript())
        A48, M48, U48 = (bytes.fromhex(k.raw[key]) for key in ("A", "M", "crs_U"))

        def refused(want, ell=4, nb=4, P=1, **edit):
            a = raw_args(k, P)
            a.update(edit)
            st = ctypes.create_string_buffer(start * P, 208 * P)
            out = ctypes.create_string_buffer(b"\xaa" * (pb * P), pb * P)
            assert call_raw(N, ctxh, tabh, ell, nb, P, a, st, out) == want, edit.keys()
            assert out.raw == b"\xaa" * (pb * P) and st.raw == start * P

        def good():
            st = ctypes.create_string_buffer(start, 208)
            out = ctypes.create_string_buffer(pb)
            assert call_raw(N, ctxh, tabh, 4, 4, 1, raw_args(k), st, out) == N.OK
            assert out.raw.hex() == k.raw["proof"] and st.raw != start

        good()
        # ---- what only the chain can see: its status word, read at its end
        refused(N.ERR_ARG, am=U48 + M48)                                                          # A not the commitment
        good()
        refused(N.ERR_ARG, am=A48 + A48)                                                          # M not the commitment
        good()
        refused(N.ERR_ARG, P=2, am=A48 + M48 + U48 + M48)                                         # one bad prover refuses the call
        good()
        ri, cb = [int(x) for x in k.r], [int(x) for x in k.cbl]
        ri[-1] = ri[-2] * cb[-1] * pow(cb[-2], -1, R) % R                                         # the constructed zero denominator
        zero_den = b"".join(x.to_bytes(32, "little") for x in ri)
        refused(N.ERR_ARG, r=zero_den)
        good()
        # ---- before anything is written
        cbl0 = bytearray(raw_args(k)["cbl"])
        cbl0[-64:-32] = bytes(32)
        refused(N.ERR_ARG, cbl=bytes(cbl0))                                                       # c[n-2] = 0, caught on the host
        for at in (0, 3):
            perm = list(k.perm)
            perm[at] = 4
            refused(N.ERR_ARG, perm=(ctypes.c_uint32 * 4)(*perm))                                 # perm entry = ell
        refused(N.ERR_ARG, gi=(ctypes.c_uint32 * n)(*([0] * (n - 1) + [len(k.table)])))
        refused(N.ERR_ARG, ui=(ctypes.c_uint32 * 1)(len(k.table)))
        for key in ("a", "abl", "mbl", "cbl", "r", "zh"):
            buf = bytearray(raw_args(k)[key])
            buf[-32:] = R.to_bytes(32, "little")
            refused(N.ERR_ENCODING, **{key: bytes(buf)})
        refused(N.ERR_ENCODING, am=bytes([A48[0] & 0x7F]) + A48[1:] + M48)                         # A with its compression flag cleared
        refused(N.ERR_ENCODING, am=A48 + bytes([M48[0] & 0x7F]) + M48[1:])
        for ell, nb in ((0, 4), (7, 1), (3, 3), (5, 2), (4092, 4)):
            refused(N.ERR_ARG, ell=ell, nb=nb)
        refused(N.ERR_ARG, P=N.IPA_MAX_PROVERS + 1)
        good()
        # ---- the Python face: refusals raise, each with its own text, and leave the caller's transcript alone
        t = k.transcript()
        pr = k.prover()
        edit = lambda at, v: pr[:at] + (v,) + pr[at + 1:]
        with pytest.raises(N.NativeError, match="A is not the commitment"):
            same_permutation_prove_device(k.table, *edit(3, k.U), t)
        with pytest.raises(N.NativeError, match="M is not the commitment"):
            same_permutation_prove_device(k.table, *edit(4, k.A), t)
        with pytest.raises(N.NativeError, match="second denominator"):
            same_permutation_prove_device(k.table, *edit(10, [Scalar(x) for x in ri]), t)
        with pytest.raises(N.NativeError, match="is zero"):
            same_permutation_prove_device(k.table, *edit(9, k.cbl[:2] + [Scalar(0)] + k.cbl[3:]), t)
        with pytest.raises(N.NativeError, match="permutation entry is >= ell"):
            same_permutation_prove_device(k.table, *edit(6, [0, 1, 2, 4]), t)
        with pytest.raises(N.NativeError, match="A does not decode"):
            same_permutation_prove_device(k.table, *edit(3, bytes([A48[0] & 0x7F]) + A48[1:]), t)
        with pytest.raises(ValueError):
            same_permutation_prove_device(k.table, k.G[:3], k.H[:3], k.U, k.A, k.M, k.a[:3], k.perm[:3], k.abl[:3], k.mbl[:3], k.cbl[:3], k.r[:6], k.zh[:4], t)
        with pytest.raises(ValueError):
            same_permutation_prove_device(k.table, *edit(11, k.zh[:-1]), t)
        with pytest.raises(ValueError):
            same_permutation_prove_device(k.table, *edit(6, k.perm[:-1]), t)
        with pytest.raises(ValueError):
            same_permutation_prove_device(k.table, *edit(8, k.mbl[:-1]), t)
        with pytest.raises(ValueError):
            same_permutation_prove_device_many(k.table, [pr], [])
        assert state(t) == start
        assert to_bytes(same_permutation_prove_device(k.table, *pr, t)).hex() == k.raw["proof"]   # the next valid call is correct
        assert fr32(t.get_and_append_challenge(b"after")).hex() == k.raw["after"]
        assert same_permutation_prove_device_many(k.table, [], []) == []
    finally:
        k.table.close()


def test_between_the_other_chains_on_one_table(native_lib, cases):
    """ipa | same-permutation | same-MSM | same-permutation (28, 4: the staging block regrows) | grand-product | same-permutation on ONE
    table handle: every call lays the shared staging block out afresh and gives its fixture's bytes and state -- the grand-product entry
    among them, whose body the same-permutation entry shares."""
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.merlin import CurdleproofsTranscript
    from curdleproofs_pie_amd.prover_kernels import grand_product_prove_device, ipa_prove_device, same_msm_prove_device, same_permutation_prove_device

    ic = next(c for c in golden("ipa_device_vectors.json") if c["n"] == 8 and c["form"] == "explicit")
    sc = next(c for c in golden("same_msm_device_vectors.json") if c["n"] == 8)
    gc = next(c for c in golden("grand_product_device_vectors.json") if (c["ell"], c["n_blinders"]) == (4, 4))
    vec = lambda case, key: [S(h) for h in case[key]]
    pts = lambda case, key: [P(h) for h in case[key]]
    ipa = (pts(ic, "crs_G_vec"), pts(ic, "crs_G_prime_vec"), P(ic["crs_H"]), P(ic["C"]), P(ic["D"]), S(ic["z"]),
           vec(ic, "vec_c"), vec(ic, "vec_d"), vec(ic, "vec_r_c"), vec(ic, "vec_r_d"))
    smsm = (pts(sc, "crs_G_vec"), P(sc["A"]), P(sc["Z_t"]), P(sc["Z_u"]), pts(sc, "vec_T"), pts(sc, "vec_U"), vec(sc, "vec_x"), vec(sc, "vec_r"))
    gprod = (pts(gc, "crs_G_vec"), pts(gc, "crs_H_vec"), P(gc["crs_U"]), P(gc["B"]), S(gc["gprod_result"]), vec(gc, "vec_b"), vec(gc, "vec_b_blinders"),
             vec(gc, "vec_c_blinders"), vec(gc, "ipa_r"), vec(gc, "ipa_z_head"))
    sp = {w: Case(cases[w], own_table=False) for w in (3, 4)}
    table = FixedBaseTable(ipa[0] + ipa[1] + [ipa[2]] + smsm[0] + gprod[0] + gprod[1] + [gprod[2]] + [b for k in sp.values() for b in k.G + k.H + [k.U]])
    for k in sp.values():
        k.table = table

    def start(case):
        t = CurdleproofsTranscript(case["label"].encode())
        t.append(case["prefix_label"].encode(), bytes.fromhex(case["prefix"]))
        return t

    def flat(res):
        out = b""
        for f in res:
            for v in f if isinstance(f, list) else [f]:
                out += bytes(v.to_compressed_bytes()) if hasattr(v, "to_compressed_bytes") else fr32(v)
        return out

    def run_ipa():
        t = start(ic)
        assert flat(ipa_prove_device(table, *ipa, t)).hex() == ic["proof"]
        assert fr32(t.get_and_append_challenge(b"after")).hex() == ic["after"]

    def run_smsm():
        t = start(sc)
        assert flat(same_msm_prove_device(table, *smsm, t)).hex() == sc["proof"]
        assert fr32(t.get_and_append_challenge(b"after")).hex() == sc["after"]

    def run_gprod():
        t = start(gc)
        assert gprod_bytes(grand_product_prove_device(table, *gprod, t)).hex() == gc["proof"]
        assert fr32(t.get_and_append_challenge(b"after")).hex() == gc["after"]

    def run_sp(w):
        k = sp[w]
        t = k.transcript()
        assert to_bytes(same_permutation_prove_device(table, *k.prover(), t)).hex() == k.raw["proof"], w
        assert fr32(t.get_and_append_challenge(b"after")).hex() == k.raw["after"], w

    try:
        run_ipa()
        run_sp(3)
        run_smsm()
        run_sp(4)
        run_gprod()
        run_sp(3)
    finally:
        table.close()
