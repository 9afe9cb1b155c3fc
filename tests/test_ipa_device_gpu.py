"""prover_kernels.ipa_prove_device / cg1_ipa_prove_device (csrc/kernels_ipa.h): the whole inner-product argument as one launch chain.
Needs an MI355X.

Pinned to the reference's bytes: tests/golden/ipa_device_vectors.json records IPA.new run stand-alone (proof bytes, and a challenge
drawn after it that pins the final transcript state).  Provers in step must each get what they get alone; edge inputs are compared
with the host-driven path (`ipa_rounds(..., table=)` with the host transcript, which the reference's recorded rounds pin in
tests/test_fixed_base_gpu.py); every refusal leaves the outputs and the transcript alone."""
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


@pytest.fixture(scope="module")
def cases(native_lib):
    return json.load(open(os.path.join(ROOT, "tests", "golden", "ipa_device_vectors.json")))["cases"]


class Case:
    """A fixture case as product objects, with its table."""

    def __init__(self, case):
        from curdleproofs_pie_amd.fixed_base import FixedBaseTable
        from curdleproofs_pie_amd.prover_kernels import grand_product_coeffs

        self.raw, self.n = case, case["n"]
        self.G, self.H = [P(h) for h in case["crs_G_vec"]], P(case["crs_H"])
        if case["form"] == "coeffs":
            self.Gp, self.coeffs = self.G, grand_product_coeffs(self.n, 0, S(case["beta_inv"]))
            self.table = FixedBaseTable(self.G + [self.H])
        else:
            self.Gp, self.coeffs = [P(h) for h in case["crs_G_prime_vec"]], None
            self.table = FixedBaseTable(self.G + self.Gp + [self.H])
        self.C, self.D, self.z = P(case["C"]), P(case["D"]), S(case["z"])
        self.c, self.d = [S(h) for h in case["vec_c"]], [S(h) for h in case["vec_d"]]
        self.rc, self.rd = [S(h) for h in case["vec_r_c"]], [S(h) for h in case["vec_r_d"]]

    def transcript(self, prefix=None):
        from curdleproofs_pie_amd.merlin import CurdleproofsTranscript

        t = CurdleproofsTranscript(self.raw["label"].encode())
        t.append(self.raw["prefix_label"].encode(), bytes.fromhex(self.raw["prefix"]) if prefix is None else prefix)
        return t

    def prover(self, rot=0):
        r = lambda v, k: v[k % self.n:] + v[:k % self.n]
        pr = (self.G, self.Gp, self.H, self.C, self.D, self.z, r(self.c, rot), r(self.d, 2 * rot), r(self.rc, 3 * rot), r(self.rd, rot))
        return pr + ((self.coeffs,) if self.coeffs is not None else ())


def to_bytes(res):
    """IPA.to_bytes order (ipa.py: B_c | B_d | vec_L_C | vec_R_C | vec_L_D | vec_R_D | c_final | d_final)."""
    B_c, B_d, LC, RC, LD, RD, c_fin, d_fin = res
    return b"".join(bytes(p.to_compressed_bytes()) for p in [B_c, B_d] + LC + RC + LD + RD) + fr32(c_fin) + fr32(d_fin)


def state(t):
    return bytes(t.strobe._st.raw)


def host_driven(table, G, Gp, crs_H, C, D, z, c, d, rc, rd, transcript, coeffs=None):
    """IPA.new after the blinder draw, driven from the host: table.msm_many, the host transcript, ipa_rounds(table=)."""
    from curdleproofs_pie_amd.prover_kernels import ipa_rounds

    k = coeffs if coeffs is not None else None
    B_c, B_d = table.msm_many([(G, rc), (Gp, rd if k is None else [a * b for a, b in zip(rd, k)])])
    comp = lambda pts: [bytes(p.to_compressed_bytes()) for p in pts]
    transcript.append_list(b"ipa_step1", comp([C, D]))
    transcript.append(b"ipa_step1", fr32(z))
    transcript.append_list(b"ipa_step1", comp([B_c, B_d]))
    alpha = transcript.get_and_append_challenge(b"ipa_alpha")
    beta = transcript.get_and_append_challenge(b"ipa_beta")
    c2 = [r + alpha * x for r, x in zip(rc, c)]
    d2 = [r + alpha * x for r, x in zip(rd, d)]

    def next_gamma(L_C, L_D, R_C, R_D):
        transcript.append_list(b"ipa_loop", comp([L_C, L_D, R_C, R_D]))
        return transcript.get_and_append_challenge(b"ipa_gamma")

    return (B_c, B_d) + tuple(ipa_rounds(G, Gp, crs_H, c2, d2, next_gamma, G_prime_coeffs=k, H_coeff=beta, table=table))


@pytest.mark.parametrize("which", range(6))
def test_fixture_cases_reproduce_reference_bytes(cases, which):
    from curdleproofs_pie_amd.prover_kernels import ipa_prove_device

    k = Case(cases[which])
    try:
        t = k.transcript()
        res = ipa_prove_device(k.table, *k.prover()[:10], t, G_prime_coeffs=k.coeffs)
        assert to_bytes(res).hex() == k.raw["proof"], (k.n, k.raw["form"])
        assert fr32(t.get_and_append_challenge(b"after")).hex() == k.raw["after"]
        # again: the same bytes, the same state
        t2 = k.transcript()
        assert to_bytes(ipa_prove_device(k.table, *k.prover()[:10], t2, G_prime_coeffs=k.coeffs)).hex() == k.raw["proof"]
        assert fr32(t2.get_and_append_challenge(b"after")).hex() == k.raw["after"]
        # and the host-driven path agrees on both
        t3 = k.transcript()
        assert to_bytes(host_driven(k.table, *k.prover()[:10], t3, k.coeffs)).hex() == k.raw["proof"]
        assert state(t3) != state(k.transcript())
        assert fr32(t3.get_and_append_challenge(b"after")).hex() == k.raw["after"]
    finally:
        k.table.close()


@pytest.mark.parametrize("which", [1, 2, 4])
def test_provers_in_step(cases, which):
    """Batches of 1, 3, 8 and 64 provers at n = 8 (both G' forms) and n = 32: rotated vectors, different transcript prefixes; prover 0 is
    the fixture's; every prover's bytes and final state equal what it gets alone."""
    from curdleproofs_pie_amd.prover_kernels import ipa_prove_device_many

    k = Case(cases[which])
    assert k.n in (8, 32)
    try:
        alone = {}
        for batch in (1, 3, 8, 64):
            provers = [k.prover(rot=i) for i in range(batch)]
            prefix = lambda i: None if i == 0 else b"prover %d" % i
            ts = [k.transcript(prefix(i)) for i in range(batch)]
            got = ipa_prove_device_many(k.table, provers, ts)
            assert len(got) == batch
            assert to_bytes(got[0]).hex() == k.raw["proof"] and fr32(ts[0].get_and_append_challenge(b"after")).hex() == k.raw["after"]
            for i in range(1, batch):
                if i not in alone:
                    t1 = k.transcript(prefix(i))
                    alone[i] = (to_bytes(ipa_prove_device_many(k.table, [provers[i]], [t1])[0]), state(t1))
                assert (to_bytes(got[i]), state(ts[i])) == alone[i], (batch, i)
            assert len({to_bytes(g) for g in got}) == batch
    finally:
        k.table.close()


def test_edge_inputs_against_the_host_driven_path(native_lib):
    """Seeded random inputs: an all-zero vec_d (identity outputs, absorbed as C0 00 ..), repeated base indices, a base outside G1,
    small scalars -- the device chain and the host-driven rounds give the same bytes and the same transcript."""
    from curdleproofs_pie_amd import G1Point, Scalar
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.merlin import CurdleproofsTranscript
    from curdleproofs_pie_amd.prover_kernels import ipa_prove_device

    rng = random.Random(7001)
    tors = json.load(open(os.path.join(ROOT, "tests", "golden", "torsion_vectors.json")))
    T3 = O.g1_decompress(bytes.fromhex(tors["t3"]))
    assert not O.g1_in_subgroup(T3)
    n = 16
    pts = [O.g1_mul(O.G1_GEN, rng.randrange(1, R)) for _ in range(2 * n + 1)]
    pts[5] = O.g1_add(T3, pts[5])                                        # order 3 r: outside G1
    objs = [G1Point.from_compressed_bytes_unchecked(O.g1_compress(p)) for p in pts]
    tab = FixedBaseTable(objs)
    rs = lambda m: [Scalar(rng.randrange(R)) for _ in range(m)]
    zero = [Scalar(0)] * n
    small = lambda m: [Scalar(rng.randrange(4)) for _ in range(m)]
    shapes = {
        "zero d": (list(range(n)), list(range(n, 2 * n)), rs(n), zero, rs(n), zero, None),
        "repeated bases": ([3] * n, [n + 1, n + 1] * (n // 2), rs(n), rs(n), rs(n), rs(n), None),
        "outside G1": (list(range(n)), list(range(n)), rs(n), rs(n), rs(n), rs(n), rs(n)),      # index 5 in both vectors, with coefficients
        "small scalars": (list(range(n)), list(range(n, 2 * n)), small(n), small(n), small(n), small(n), None),
        "all zero": (list(range(n)), list(range(n, 2 * n)), zero, zero, zero, zero, None),
    }
    try:
        for name, (gi, gpi, c, d, rc, rd, coeffs) in shapes.items():
            G, Gp, H = [objs[i] for i in gi], [objs[i] for i in gpi], objs[2 * n]
            C, D = tab.msm(c, G), tab.msm(d, Gp)
            z = Scalar(sum(int(a) * int(b) for a, b in zip(c, d)) % R)
            mk = lambda: CurdleproofsTranscript(b"edge " + name.encode())
            t_dev, t_host = mk(), mk()
            # bases as indices on the device path, as objects on the host-driven one
            got = ipa_prove_device(tab, gi, gpi, 2 * n, C, D, z, c, d, rc, rd, t_dev, G_prime_coeffs=coeffs)
            want = host_driven(tab, G, Gp, H, C, D, z, c, d, rc, rd, t_host, coeffs)
            assert to_bytes(got) == to_bytes(want), name
            assert state(t_dev) == state(t_host), name
            if name in ("zero d", "all zero"):
                inf = b"\xc0" + bytes(47)
                assert bytes(got[1].to_compressed_bytes()) == inf and all(bytes(p.to_compressed_bytes()) == inf for p in got[4] + got[5]), name
    finally:
        tab.close()


def raw_args(k, P=1):
    """The C entry's arguments for P copies of a fixture case (explicit form)."""
    n = k.n
    gi = (ctypes.c_uint32 * (n * P))(*(list(range(n)) * P))
    gpi = (ctypes.c_uint32 * (n * P))(*(list(range(n, 2 * n)) * P))
    hi = (ctypes.c_uint32 * P)(*([2 * n] * P))
    cd = (bytes.fromhex(k.raw["C"]) + bytes.fromhex(k.raw["D"])) * P
    vec = lambda key: b"".join(bytes.fromhex(h) for h in k.raw[key]) * P
    return dict(gi=gi, gpi=gpi, hi=hi, coef=None, cd=cd, z=bytes.fromhex(k.raw["z"]) * P, c=vec("vec_c"), d=vec("vec_d"), rc=vec("vec_r_c"), rd=vec("vec_r_d"))


def call_raw(N, ctx_handle, tab_handle, n, P, a, st, out):
    return N.cg1_ipa_prove_device(ctx_handle, tab_handle, n, P, a["gi"], a["gpi"], a["hi"], a["coef"], a["cd"], a["z"], a["c"], a["d"], a["rc"], a["rd"], st, out, None)


def test_refusals_leave_everything_untouched(native_lib, cases):
    from curdleproofs_pie_amd import Scalar
    from curdleproofs_pie_amd.prover_kernels import ipa_prove_device, ipa_prove_device_many

    N = native_lib
    k = Case(cases[1])                                                    # n = 8, explicit G'
    n, pb = k.n, 736
    try:
        ctxh, tabh = k.table._ctx.handle, k.table._tab.handle
        start = state(k.transcript())

        def refused(want, n_=n, P=1, **edit):
            a = raw_args(k, P)
            a.update(edit)
            st = ctypes.create_string_buffer(start * P, 208 * P)
            out = ctypes.create_string_buffer(b"\xaa" * (pb * P), pb * P)
            assert call_raw(N, ctxh, tabh, n_, P, a, st, out) == want, edit.keys()
            assert out.raw == b"\xaa" * (pb * P) and st.raw == start * P

        def good():
            a = raw_args(k)
            st = ctypes.create_string_buffer(start, 208)
            out = ctypes.create_string_buffer(pb)
            assert call_raw(N, ctxh, tabh, n, 1, a, st, out) == N.OK
            assert out.raw.hex() == k.raw["proof"] and st.raw != start

        good()
        for bad_n in (0, 1, 3, 6, 4096):
            refused(N.ERR_ARG, n_=bad_n)
        refused(N.ERR_ARG, P=N.IPA_MAX_PROVERS + 1)
        good()
        bad_idx = (ctypes.c_uint32 * n)(*([0] * (n - 1) + [len(k.table)]))
        refused(N.ERR_ARG, gi=bad_idx)
        refused(N.ERR_ARG, gpi=bad_idx)
        refused(N.ERR_ARG, hi=(ctypes.c_uint32 * 1)(len(k.table)))
        refused(N.ERR_ARG, gi=(ctypes.c_uint32 * n)(*([0] * (n - 1) + [1 << 31])))             # no negated bases here
        good()
        for key in ("z", "c", "d", "rc", "rd"):
            for bad in (R, (1 << 256) - 1):
                a = raw_args(k)
                buf = bytearray(a[key])
                buf[-32:] = bad.to_bytes(32, "little")
                refused(N.ERR_ENCODING, **{key: bytes(buf)})
        refused(N.ERR_ENCODING, coef=(1).to_bytes(32, "little") * (n - 1) + R.to_bytes(32, "little"))
        good()
        cd = raw_args(k)["cd"]
        refused(N.ERR_ENCODING, cd=bytes([cd[0] & 0x7F]) + cd[1:])                               # C without the compression flag
        refused(N.ERR_ENCODING, cd=cd[:48] + b"\x9f" + b"\xff" * 47)                             # D with x >= p
        off_curve = next(x for x in range(1, 50) if pow((x ** 3 + 4) % O.P, (O.P - 1) // 2, O.P) != 1)
        refused(N.ERR_NOT_ON_CURVE, cd=cd[:48] + bytes([0x80 | (off_curve >> 376)]) + off_curve.to_bytes(48, "big")[1:])
        good()
        # a table of another context on the same device is fine; a closed one is not reached (the Python face raises first)
        # ---- the Python face: refusals raise and leave the caller's transcript alone
        t = k.transcript()
        with pytest.raises(ValueError):
            ipa_prove_device(k.table, k.G[:6], k.Gp[:6], k.H, k.C, k.D, k.z, k.c[:6], k.d[:6], k.rc[:6], k.rd[:6], t)
        with pytest.raises(ValueError):
            ipa_prove_device(k.table, k.G[:1], k.Gp[:1], k.H, k.C, k.D, k.z, k.c[:1], k.d[:1], k.rc[:1], k.rd[:1], t)
        with pytest.raises(KeyError):
            ipa_prove_device(k.table, k.G, k.Gp, P(k.raw["crs_H"]), k.C, k.D, k.z, k.c, k.d, k.rc, k.rd, t)
        with pytest.raises(IndexError):
            ipa_prove_device(k.table, list(range(n - 1)) + [len(k.table)], k.Gp, k.H, k.C, k.D, k.z, k.c, k.d, k.rc, k.rd, t)
        with pytest.raises(N.NativeError):
            ipa_prove_device(k.table, k.G, k.Gp, k.H, k.C, k.D, k.z, k.c[:-1] + [R], k.d, k.rc, k.rd, t)       # a plain int >= r
        with pytest.raises(N.NativeError):
            ipa_prove_device(k.table, k.G, k.Gp, k.H, b"\x00" * 48, k.D, k.z, k.c, k.d, k.rc, k.rd, t)
        with pytest.raises(ValueError):
            ipa_prove_device_many(k.table, [k.prover()], [])
        assert state(t) == start
        assert to_bytes(ipa_prove_device(k.table, *k.prover(), t)).hex() == k.raw["proof"]                          # the next valid call is correct
        assert fr32(t.get_and_append_challenge(b"after")).hex() == k.raw["after"]
        assert ipa_prove_device_many(k.table, [], []) == []
    finally:
        k.table.close()
    with pytest.raises(N.NativeError):
        ipa_prove_device(k.table, *k.prover(), k.transcript())                                                     # the table is closed


def test_both_inversions_give_the_same_bytes(native_lib, cases):
    """ "ipa_inv" is an A/B switch of the round challenge's inversion (binary Euclid / a^(r-2)): the same proof either way."""
    from curdleproofs_pie_amd.prover_kernels import ipa_prove_device

    k = Case(cases[2])
    try:
        ctx = k.table._ctx
        for mode in (1, 0):
            ctx.set_param("ipa_inv", mode)
            t = k.transcript()
            assert to_bytes(ipa_prove_device(k.table, *k.prover(), t)).hex() == k.raw["proof"], mode
            assert fr32(t.get_and_append_challenge(b"after")).hex() == k.raw["after"]
        with pytest.raises(native_lib.NativeError):
            ctx.set_param("ipa_inv", 2)
    finally:
        k.table._ctx.set_param("ipa_inv", 0)
        k.table.close()
