"""prover_kernels.grand_product_prove_device / cg1_gprod_prove_device (csrc/kernels_gprod.h, then the phases of csrc/kernels_ipa.h): the whole
grand-product argument as one launch chain.  Needs an MI355X.

Pinned to the reference's bytes: tests/golden/grand_product_device_vectors.json records GrandProductProof.new run stand-alone (proof bytes,
and a challenge drawn after it that pins the final transcript state).  Provers in step must each get what they get alone; edge inputs are
compared with a host-driven path written here (Python ints, table.msm_many, the host transcript, then ipa_prove_device with
G_prime_coeffs); every refusal leaves the outputs and the transcript alone; and a grand-product call between an inner-product and a
same-MSM call on one table handle shares their staging block."""
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
    return golden("grand_product_device_vectors.json")


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
        self.B, self.gres = P(case["B"]), S(case["gprod_result"])
        vec = lambda key: [S(h) for h in case[key]]
        self.b, self.bbl, self.cbl, self.r, self.zh = vec("vec_b"), vec("vec_b_blinders"), vec("vec_c_blinders"), vec("ipa_r"), vec("ipa_z_head")

    def transcript(self, prefix=None):
        from curdleproofs_pie_amd.merlin import CurdleproofsTranscript

        t = CurdleproofsTranscript(self.raw["label"].encode())
        t.append(self.raw["prefix_label"].encode(), bytes.fromhex(self.raw["prefix"]) if prefix is None else prefix)
        return t

    def prover(self, rot=0):
        """Prover `rot` of a call in step: rotated vectors and one changed b, so B and gprod_result are its own (recomputed here)."""
        from curdleproofs_pie_amd import Scalar

        if rot == 0:
            return (self.G, self.H, self.U, self.B, self.gres, self.b, self.bbl, self.cbl, self.r, self.zh)
        r = lambda v, k: v[k % len(v):] + v[:k % len(v)]
        b = r(self.b, rot)
        b[0] = b[0] + Scalar(rot)
        bbl = r(self.bbl, rot)
        prod = 1
        for x in b:
            prod = prod * int(x) % R
        B = self.table.msm(b + bbl, list(self.G) + list(self.H))
        return (self.G, self.H, self.U, B, Scalar(prod), b, bbl, r(self.cbl, 2 * rot), r(self.r, 3 * rot), r(self.zh, rot))


def to_bytes(res):
    """GrandProductProof.to_bytes: C | r_p | IPA.to_bytes (B_c | B_d | vec_L_C | vec_R_C | vec_L_D | vec_R_D | c_final | d_final)."""
    C, r_p, (B_c, B_d, LC, RC, LD, RD, c_fin, d_fin) = res
    comp = lambda p: bytes(p.to_compressed_bytes())
    return comp(C) + fr32(r_p) + b"".join(comp(p) for p in [B_c, B_d] + LC + RC + LD + RD) + fr32(c_fin) + fr32(d_fin)


def state(t):
    return bytes(t.strobe._st.raw)


def host_driven(table, G, H, U, B, gres, b, bbl, cbl, r, zh, transcript):
    """GrandProductProof.new after its draws, driven from the host: Python ints, table.msm_many, the host transcript, the completion of
    generate_ipa_blinders (ipa.py:33-41), then ipa_prove_device with the base change as G_prime_coeffs."""
    from curdleproofs_pie_amd import G1Point, Scalar
    from curdleproofs_pie_amd.prover_kernels import grand_product_coeffs, ipa_prove_device

    ell, nb = len(G), len(H)
    n = ell + nb
    vec_G = list(G) + list(H)
    comp = lambda p: bytes(p.to_compressed_bytes()) if type(p) is G1Point else bytes(p)
    bi, bbi, cbi, ri, zi, gr = ([int(x) for x in v] for v in (b, bbl, cbl, r, zh, [gres]))
    transcript.append(b"gprod_step1", comp(B))
    transcript.append(b"gprod_step1", fr32(gres))
    alpha = int(transcript.get_and_append_challenge(b"gprod_alpha"))
    c = [1]
    for i in range(ell - 1):
        c.append(c[i] * bi[i] % R)
    c += cbi
    (C,) = table.msm_many([(vec_G, [Scalar(x) for x in c])])
    rba = [(x + alpha) % R for x in bbi]
    r_p = sum(x * y for x, y in zip(rba, cbi)) % R
    transcript.append(b"gprod_step2", comp(C))
    transcript.append(b"gprod_step2", fr32(Scalar(r_p)))
    beta = int(transcript.get_and_append_challenge(b"gprod_beta"))
    beta_inv = pow(beta, -1, R)
    kgp = [int(x) for x in grand_product_coeffs(ell, nb, Scalar(beta_inv))]
    d = [(bi[j] * pow(beta, j + 1, R) - pow(beta, j, R)) % R for j in range(ell)] + [pow(beta, ell + 1, R) * x % R for x in rba]
    (D,) = table.msm_many([(vec_G, [Scalar(x * k % R) for x, k in zip(d, kgp)])])
    inner = (r_p * pow(beta, ell + 1, R) + gr[0] * pow(beta, ell, R) - 1) % R
    dot = lambda u, v: sum(x * y for x, y in zip(u, v)) % R
    omega, delta = (dot(ri, d) + dot(zi, c[: n - 2])) % R, dot(ri[: n - 2], zi)
    inv_c = pow(c[n - 2], -1, R)
    last_z = (ri[n - 2] * inv_c * omega - delta) * pow((-ri[n - 2] * inv_c * c[n - 1] + ri[n - 1]) % R, -1, R) % R
    pen_z = -inv_c * (last_z * c[n - 1] + omega) % R
    z = zi + [pen_z, last_z]
    sc = lambda v: [Scalar(x) for x in v]
    ipa = ipa_prove_device(table, vec_G, vec_G, U, C, D, Scalar(inner), sc(c), sc(d), sc(ri), sc(z), transcript, G_prime_coeffs=sc(kgp))
    return (C, Scalar(r_p), ipa)


@pytest.fixture(scope="module")
def big(cases):
    """The (508, 4) case with its table of 513 bases: shared with the ell = 300 edge input."""
    k = Case(cases[6])
    yield k
    k.table.close()


@pytest.mark.parametrize("which", range(7))
def test_fixture_cases_reproduce_reference_bytes(cases, big, which):
    from curdleproofs_pie_amd.prover_kernels import grand_product_prove_device

    k = big if which == 6 else Case(cases[which])
    try:
        for _ in range(2):                                               # again: the same bytes, the same state
            t = k.transcript()
            res = grand_product_prove_device(k.table, *k.prover(), t)
            assert to_bytes(res).hex() == k.raw["proof"], (k.ell, k.nb)
            assert state(t) != state(k.transcript())
            assert fr32(t.get_and_append_challenge(b"after")).hex() == k.raw["after"]
    finally:
        if k is not big:
            k.table.close()


@pytest.mark.parametrize("which", [3, 4])
def test_provers_in_step(cases, which):
    """Batches of 1, 3, 8 and 64 provers at (4, 4) and (28, 4): rotated vectors, their own B and gprod_result, different transcript
    prefixes; prover 0 is the fixture's; every prover's bytes and final state equal what it gets alone."""
    from curdleproofs_pie_amd.prover_kernels import grand_product_prove_device_many

    k = Case(cases[which])
    assert (k.ell, k.nb) in ((4, 4), (28, 4))
    try:
        alone = {}
        all_provers = [k.prover(rot=i) for i in range(64)]
        for batch in (1, 3, 8, 64):
            provers = all_provers[:batch]
            prefix = lambda i: None if i == 0 else b"prover %d" % i
            ts = [k.transcript(prefix(i)) for i in range(batch)]
            got = grand_product_prove_device_many(k.table, provers, ts)
            assert len(got) == batch
            assert to_bytes(got[0]).hex() == k.raw["proof"] and fr32(ts[0].get_and_append_challenge(b"after")).hex() == k.raw["after"]
            for i in range(1, batch):
                if i not in alone:
                    t1 = k.transcript(prefix(i))
                    alone[i] = (to_bytes(grand_product_prove_device_many(k.table, [provers[i]], [t1])[0]), state(t1))
                assert (to_bytes(got[i]), state(ts[i])) == alone[i], (batch, i)
            assert len({to_bytes(g) for g in got}) == batch
    finally:
        k.table.close()


def test_edge_inputs_against_the_host_driven_path(native_lib, big):
    """Seeded random inputs: some b_i = 0 (gprod_result = 0, a zero tail of vec_c), repeated base indices, a base outside G1, and
    ell = 300 (n = 512: a second scan shape, 212 blinders) over the big table -- the device chain and the host-driven path give the
    same bytes and the same transcript."""
    from curdleproofs_pie_amd import G1Point, Scalar
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.merlin import CurdleproofsTranscript
    from curdleproofs_pie_amd.prover_kernels import grand_product_prove_device

    rng = random.Random(7101)
    tors = golden_raw("torsion_vectors.json")
    T3 = O.g1_decompress(bytes.fromhex(tors["t3"]))
    assert not O.g1_in_subgroup(T3)
    n = 16
    pts = [O.g1_mul(O.G1_GEN, rng.randrange(1, R)) for _ in range(n + 1)]
    pts[5] = O.g1_add(T3, pts[5])                                        # order 3 r: outside G1
    objs = [G1Point.from_compressed_bytes_unchecked(O.g1_compress(p)) for p in pts]
    tab = FixedBaseTable(objs)
    rs = lambda m: [Scalar(rng.randrange(1, R)) for _ in range(m)]
    with_zero = rs(12)
    with_zero[4] = Scalar(0)
    with_zero[9] = Scalar(0)
    shapes = {
        "zero b": (tab, list(range(12)), list(range(12, 16)), n, with_zero),
        "repeated bases": (tab, [3] * 12, [13, 13, 14, 3], 3, rs(12)),
        "outside G1": (tab, list(range(14)), [14, 15], n, rs(14)),                              # index 5 is among crs_G_vec
        "ell 300": (big.table, list(range(300)), list(range(300, 512)), 512, rs(300)),
    }
    try:
        for name, (table, gi, hi, ui, b) in shapes.items():
            ell, nb = len(gi), len(hi)
            m = ell + nb
            bbl, cbl, r, zh = rs(nb), rs(nb), rs(m), rs(m - 2)
            prod = 1
            for x in b:
                prod = prod * int(x) % R
            gres = Scalar(prod)
            B = table.msm(b + bbl, gi + hi)
            mk = lambda: CurdleproofsTranscript(b"edge " + name.encode())
            t_dev, t_host = mk(), mk()
            keep = [list(v) for v in (b, bbl, cbl, r, zh)]
            got = grand_product_prove_device(table, gi, hi, ui, B, gres, b, bbl, cbl, r, zh, t_dev)
            assert [list(v) for v in (b, bbl, cbl, r, zh)] == keep, name                       # no input is mutated
            want = host_driven(table, gi, hi, ui, B, gres, b, bbl, cbl, r, zh, t_host)
            assert to_bytes(got) == to_bytes(want), name
            assert state(t_dev) == state(t_host), name
            if name == "zero b":
                assert prod == 0
    finally:
        tab.close()


def raw_args(k, P=1):
    """The C entry's arguments for P copies of a fixture case."""
    n = k.n
    vec = lambda *keys: b"".join(bytes.fromhex(h) for key in keys for h in k.raw[key]) * P
    return dict(gi=(ctypes.c_uint32 * (n * P))(*(list(range(n)) * P)), ui=(ctypes.c_uint32 * P)(*([n] * P)), B=bytes.fromhex(k.raw["B"]) * P,
                gres=bytes.fromhex(k.raw["gprod_result"]) * P, b=vec("vec_b", "vec_b_blinders"), cbl=vec("vec_c_blinders"), r=vec("ipa_r"), zh=vec("ipa_z_head"))


def call_raw(N, ctx_handle, tab_handle, ell, nb, P, a, st, out):
    return N.cg1_gprod_prove_device(ctx_handle, tab_handle, ell, nb, P, a["gi"], a["ui"], a["B"], a["gres"], a["b"], a["cbl"], a["r"], a["zh"], st, out, None)


def test_refusals_leave_everything_untouched(native_lib, cases):
    from curdleproofs_pie_amd import Scalar
    from curdleproofs_pie_amd.prover_kernels import grand_product_prove_device, grand_product_prove_device_many

    N = native_lib
    k = Case(cases[3])                                                    # (4, 4)
    n, pb = k.n, 816
    try:
        ctxh, tabh = k.table._ctx.handle, k.table._tab.handle
        start = state(k.transcript())

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
        refused(N.ERR_ARG, B=bytes.fromhex(k.raw["crs_U"]))                                       # B not the commitment
        good()
        refused(N.ERR_ARG, gres=((int(k.gres) + 1) % R).to_bytes(32, "little"))                   # wrong gprod_result
        good()
        ri, cb = [int(x) for x in k.r], [int(x) for x in k.cbl]
        ri[-1] = ri[-2] * cb[-1] * pow(cb[-2], -1, R) % R                                         # the constructed zero denominator
        zero_den = b"".join(x.to_bytes(32, "little") for x in ri)
        refused(N.ERR_ARG, r=zero_den)
        good()
        refused(N.ERR_ARG, P=2, B=bytes.fromhex(k.raw["B"]) + bytes.fromhex(k.raw["crs_U"]))       # one bad prover refuses the call
        good()
        # ---- before anything is written
        for ell, nb in ((0, 4), (7, 1), (3, 3), (5, 2), (4092, 4)):
            refused(N.ERR_ARG, ell=ell, nb=nb)
        refused(N.ERR_ARG, P=N.IPA_MAX_PROVERS + 1)
        refused(N.ERR_ARG, gi=(ctypes.c_uint32 * n)(*([0] * (n - 1) + [len(k.table)])))
        refused(N.ERR_ARG, ui=(ctypes.c_uint32 * 1)(len(k.table)))
        for key in ("gres", "b", "cbl", "r", "zh"):
            buf = bytearray(raw_args(k)[key])
            buf[-32:] = R.to_bytes(32, "little")
            refused(N.ERR_ENCODING, **{key: bytes(buf)})
        refused(N.ERR_ENCODING, B=bytes([bytes.fromhex(k.raw["B"])[0] & 0x7F]) + bytes.fromhex(k.raw["B"])[1:])
        cbl0 = bytearray(raw_args(k)["cbl"])
        cbl0[-64:-32] = bytes(32)
        refused(N.ERR_ARG, cbl=bytes(cbl0))                                                       # c[n-2] = 0, caught on the host
        good()
        # ---- the Python face: refusals raise, each with its own text, and leave the caller's transcript alone
        t = k.transcript()
        pr = k.prover()
        edit = lambda at, v: pr[:at] + (v,) + pr[at + 1:]
        with pytest.raises(N.NativeError, match="B is not the commitment"):
            grand_product_prove_device(k.table, *edit(3, k.U), t)
        with pytest.raises(N.NativeError, match="gprod_result is not the product"):
            grand_product_prove_device(k.table, *edit(4, k.gres + Scalar(1)), t)
        with pytest.raises(N.NativeError, match="second denominator"):
            grand_product_prove_device(k.table, *edit(8, [Scalar(x) for x in ri]), t)
        with pytest.raises(N.NativeError, match="is zero"):
            grand_product_prove_device(k.table, *edit(7, k.cbl[:2] + [Scalar(0)] + k.cbl[3:]), t)
        with pytest.raises(ValueError):
            grand_product_prove_device(k.table, k.G[:3], k.H[:3], k.U, k.B, k.gres, k.b[:3], k.bbl[:3], k.cbl[:3], k.r[:6], k.zh[:4], t)
        with pytest.raises(ValueError):
            grand_product_prove_device(k.table, *edit(9, k.zh[:-1]), t)
        with pytest.raises(ValueError):
            grand_product_prove_device_many(k.table, [pr], [])
        assert state(t) == start
        assert to_bytes(grand_product_prove_device(k.table, *pr, t)).hex() == k.raw["proof"]      # the next valid call is correct
        assert fr32(t.get_and_append_challenge(b"after")).hex() == k.raw["after"]
        assert grand_product_prove_device_many(k.table, [], []) == []
    finally:
        k.table.close()


def test_between_an_ipa_and_a_same_msm_call_on_one_table(native_lib, cases):
    """ipa | grand product | same-MSM | grand product (a larger shape: the staging block regrows) | ipa | grand product on ONE table
    handle: every call lays the shared staging block out afresh and gives the reference's bytes and state."""
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.merlin import CurdleproofsTranscript
    from curdleproofs_pie_amd.prover_kernels import grand_product_prove_device, ipa_prove_device, same_msm_prove_device

    ic = next(c for c in golden("ipa_device_vectors.json") if c["n"] == 8 and c["form"] == "explicit")
    sc = next(c for c in golden("same_msm_device_vectors.json") if c["n"] == 8)
    vec = lambda case, key: [S(h) for h in case[key]]
    ipa = ([P(h) for h in ic["crs_G_vec"]], [P(h) for h in ic["crs_G_prime_vec"]], P(ic["crs_H"]), P(ic["C"]), P(ic["D"]), S(ic["z"]),
           vec(ic, "vec_c"), vec(ic, "vec_d"), vec(ic, "vec_r_c"), vec(ic, "vec_r_d"))
    smsm = ([P(h) for h in sc["crs_G_vec"]], P(sc["A"]), P(sc["Z_t"]), P(sc["Z_u"]), [P(h) for h in sc["vec_T"]], [P(h) for h in sc["vec_U"]],
            vec(sc, "vec_x"), vec(sc, "vec_r"))
    gp = {w: Case(cases[w], own_table=False) for w in (3, 4)}
    table = FixedBaseTable(ipa[0] + ipa[1] + [ipa[2]] + smsm[0] + [b for k in gp.values() for b in k.G + k.H + [k.U]])
    for k in gp.values():
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

    def run_gp(w):
        k = gp[w]
        t = k.transcript()
        assert to_bytes(grand_product_prove_device(table, *k.prover(), t)).hex() == k.raw["proof"], w
        assert fr32(t.get_and_append_challenge(b"after")).hex() == k.raw["after"], w

    try:
        run_ipa()
        run_gp(3)
        run_smsm()
        run_gp(4)
        run_ipa()
        run_gp(3)
        run_smsm()
    finally:
        table.close()
