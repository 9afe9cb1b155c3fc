"""The device prover of the inner-product argument, the parts that run without a GPU: the scalar schedule and the folds k_ipa_step runs
(cg1_ipa_round_emulate is compiled from csrc/ipa_rounds.h, the header the kernel includes) against the reference's IPA.new as recorded
in tests/golden/ipa_device_vectors.json -- the final scalars for every case, and for the small cases every term list evaluated with the
CPU oracle against the proof's points -- plus the refusals and the symbol lists."""
import ctypes
import json
import os
import re

import pytest

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = O.R
IPA = ["cg1_ipa_proof_bytes", "cg1_ipa_prove_device", "cg1_ipa_round_emulate"]


@pytest.fixture(scope="module")
def cases():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "ipa_device_vectors.json")))["cases"]


def s32(values):
    return b"".join(v.to_bytes(32, "little") for v in values)


def ints(raw, n):
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(n)]


def le(h):
    return int.from_bytes(bytes.fromhex(h), "little")


def coeffs_of(case):
    """The G' coefficients of a case: beta^-(i+1) in the coefficient form (grand_prod.py:64-71), ones otherwise."""
    n = case["n"]
    if case["form"] != "coeffs":
        return [1] * n
    b = le(case["beta_inv"])
    return [pow(b, i + 1, R) for i in range(n)]


class Emu:
    """One prover's state driven through cg1_ipa_round_emulate."""

    def __init__(self, N, case):
        n = self.n0 = self.len = case["n"]
        self.N = N
        self.c = ctypes.create_string_buffer(s32([le(h) for h in case["vec_c"]]), 32 * n)
        self.d = ctypes.create_string_buffer(s32([le(h) for h in case["vec_d"]]), 32 * n)
        self.kg = ctypes.create_string_buffer(s32([1] * n), 32 * n)
        self.kgp = ctypes.create_string_buffer(s32(coeffs_of(case)), 32 * n)
        self.kh = s32([le(case["beta"])])
        self.rc, self.rd = s32([le(h) for h in case["vec_r_c"]]), s32([le(h) for h in case["vec_r_d"]])
        # table layout of the tests: G at 0 .. n-1, G' at n .. 2n-1 (the coefficient form points back at G), crs_H at 2n
        self.gi = (ctypes.c_uint32 * n)(*range(n))
        self.gpi = (ctypes.c_uint32 * n)(*(range(n) if case["form"] == "coeffs" else range(n, 2 * n)))
        self.hi = 2 * n

    def call(self, op, challenge=None, want=0):
        n = self.n0
        nt, nm = (2 * n, 2) if op == 0 else (2 * n + 2, 4)
        tb, sc, offs = (ctypes.c_uint32 * nt)(), ctypes.create_string_buffer(32 * nt), (ctypes.c_uint32 * (nm + 1))()
        rc = self.N.cg1_ipa_round_emulate(op, n, self.len, self.c, self.d, self.kg, self.kgp, self.kh, None if challenge is None else s32([challenge]),
                                          self.rc, self.rd, self.gi, self.gpi, self.hi, tb, sc, offs)
        assert rc == want, (op, rc)
        if op == 2 and challenge is not None and rc == 0:
            self.len //= 2
        return list(tb), ints(sc.raw, nt), list(offs)

    def vectors(self):
        return ints(self.c.raw, self.len), ints(self.d.raw, self.len)


def proof_fields(case):
    n, raw = case["n"], bytes.fromhex(case["proof"])
    lg = n.bit_length() - 1
    pts = [raw[48 * j: 48 * j + 48] for j in range(2 + 4 * lg)]
    vec = lambda q: pts[2 + q * lg: 2 + (q + 1) * lg]
    return dict(B_c=pts[0], B_d=pts[1], L_C=vec(0), R_C=vec(1), L_D=vec(2), R_D=vec(3), c_final=int.from_bytes(raw[-64:-32], "little"),
                d_final=int.from_bytes(raw[-32:], "little"))


def test_fixture_shape(cases):
    assert [(c["n"], c["form"]) for c in cases] == [(2, "explicit"), (8, "explicit"), (32, "explicit"), (128, "explicit"), (8, "coeffs"), (128, "coeffs")]
    for c in cases:
        lg = c["n"].bit_length() - 1
        assert len(c["proof"]) // 2 == (2 + 4 * lg) * 48 + 64 and len(c["gammas"]) == lg
        # z = <c, d>, and the blinders satisfy the reference's two relations (ipa.py:45-46)
        cv, dv, rc, rd = ([le(h) for h in c[k]] for k in ("vec_c", "vec_d", "vec_r_c", "vec_r_d"))
        assert sum(a * b for a, b in zip(cv, dv)) % R == le(c["z"])
        assert (sum(a * b for a, b in zip(rc, dv)) + sum(a * b for a, b in zip(rd, cv))) % R == 0 and sum(a * b for a, b in zip(rc, rd)) % R == 0


def test_final_scalars_every_case(native_lib, cases):
    """Blinding with the recorded alpha and folding with the recorded gammas gives the proof's c_final / d_final (Fr only)."""
    for case in cases:
        e = Emu(native_lib, case)
        e.call(1, le(case["alpha"]))
        alpha, cv, dv = le(case["alpha"]), [le(h) for h in case["vec_c"]], [le(h) for h in case["vec_d"]]
        assert e.vectors() == ([(r + alpha * c) % R for r, c in zip((le(h) for h in case["vec_r_c"]), cv)],
                               [(r + alpha * d) % R for r, d in zip((le(h) for h in case["vec_r_d"]), dv)])
        for g in case["gammas"]:
            e.call(2, le(g))
        want = proof_fields(case)
        assert e.len == 1 and e.vectors() == ([want["c_final"]], [want["d_final"]]), (case["n"], case["form"])


def evaluate(bases, tb, sc, lo, hi):
    acc = None
    for i in range(lo, hi):
        assert tb[i] >> 31 == 0                                          # no negated base in this schedule
        acc = O.g1_add(acc, O.g1_mul(bases[tb[i]], sc[i]))
    return O.g1_compress(acc)


@pytest.mark.parametrize("which", [0, 1, 4])
def test_term_lists_give_the_reference_points(native_lib, cases, which):
    """n = 2, n = 8 and the coefficient-form n = 8: every launch's term list, evaluated by the oracle over the fixture's bases."""
    case = cases[which]
    n = case["n"]
    assert n in (2, 8)
    dec = lambda h: O.g1_decompress(bytes.fromhex(h))
    bases = [dec(h) for h in case["crs_G_vec"]] + [dec(h) for h in case["crs_G_prime_vec"]] + [dec(case["crs_H"])]
    want = proof_fields(case)
    e = Emu(native_lib, case)
    tb, sc, offs = e.call(0)
    assert offs == [0, n, 2 * n]
    assert evaluate(bases, tb, sc, 0, n) == want["B_c"] and evaluate(bases, tb, sc, n, 2 * n) == want["B_d"]
    e.call(1, le(case["alpha"]))
    h = n // 2
    for k, g in enumerate(case["gammas"]):
        tb, sc, offs = e.call(2, le(g))
        assert offs == [0, h + 1, 2 * h + 1, 3 * h + 2, 4 * h + 2] and offs == sorted(offs)
        assert all(v < R for v in sc) and all(t < 2 * n + 1 for t in tb)
        assert tb[h] == 2 * n and tb[3 * h + 1] == 2 * n                 # the H terms close L_C and R_C
        got = [evaluate(bases, tb, sc, offs[j], offs[j + 1]) for j in range(4)]
        assert got == [want["L_C"][k], want["L_D"][k], want["R_C"][k], want["R_D"][k]], (n, k)


def test_terms_without_a_fold_leave_the_state(native_lib, cases):
    e = Emu(native_lib, cases[1])
    e.call(1, le(cases[1]["alpha"]))
    before = (e.c.raw, e.d.raw, e.kg.raw, e.kgp.raw)
    a = e.call(2)
    assert (e.c.raw, e.d.raw, e.kg.raw, e.kgp.raw) == before and e.len == 8
    assert e.call(2) == a


def test_gamma_inverse_random(native_lib, cases):
    """The kernel's inversion (Kaliski's almost-inverse, csrc/ipa_rounds.h) against Python's pow on random and edge challenges: the fold
    of a length-2 state is c0 + c1 / gamma; the entry itself also compares with a^(r-2) and refuses when they differ."""
    import random

    rng = random.Random(77)
    case = cases[0]
    c0, c1 = le(case["vec_c"][0]), le(case["vec_c"][1])
    for g in [1, 2, 3, R - 1, R - 2, (R + 1) // 2, 1 << 254, (1 << 255) - 19 - R] + [1 << k for k in range(0, 254, 23)] + [rng.randrange(1, R) for _ in range(400)]:
        e = Emu(native_lib, case)
        e.call(2, g % R)
        assert e.vectors()[0] == [(c0 + pow(g % R, -1, R) * c1) % R], hex(g)


def test_refusals(native_lib, cases):
    N = native_lib
    assert N.cg1_ipa_proof_bytes(128) == 1504 and N.cg1_ipa_proof_bytes(2) == 352 and N.cg1_ipa_proof_bytes(8) == 736
    for bad in (0, 1, 3, 6, 100):
        assert N.cg1_ipa_proof_bytes(bad) == 0
    e = Emu(N, cases[1])
    for bad in (R, R + 5, (1 << 256) - 1):                               # a scalar >= r is refused, never reduced
        e.call(1, bad, want=N.ERR_ENCODING)
        keep = e.c.raw
        e.c = ctypes.create_string_buffer(s32([bad]) + keep[32:], len(keep))
        before = e.d.raw
        e.call(2, 5, want=N.ERR_ENCODING)
        assert e.d.raw == before
        e.c = ctypes.create_string_buffer(keep, len(keep))
    e.call(2, 0, want=N.ERR_ARG)                                         # gamma = 0 has no inverse
    for n0, ln in ((6, 6), (1, 1), (8, 3), (8, 16), (12, 4)):            # not a power of two, below 2, longer than n0
        e2 = Emu(N, cases[1])
        e2.n0, e2.len = n0, ln
        e2.call(2, 5, want=N.ERR_ARG)
    e.call(1, le(cases[1]["alpha"]))                                     # and the state is still usable
    for g in cases[1]["gammas"]:
        e.call(2, le(g))
    assert e.vectors()[0] == [proof_fields(cases[1])["c_final"]]


def test_symbol_lists_agree(native_lib):
    src = open(os.path.join(ROOT, "include", "curdle_g1.h")).read()
    stripped = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cg1_[a-z0-9_]+)\s*\(", stripped))
    lib = ctypes.CDLL(native_lib.LIB_PATH)
    for name in IPA:
        assert name in declared and hasattr(lib, name) and name in native_lib.EXPORTED_SYMBOLS and callable(getattr(native_lib, name)), name
    assert sorted(native_lib.EXPORTED_SYMBOLS) == sorted(declared)
    for macro, value in (("CG1_IPA_MAX_N", native_lib.IPA_MAX_N), ("CG1_IPA_MAX_PROVERS", native_lib.IPA_MAX_PROVERS)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), stripped), macro
    # 4 MSMs per prover per launch, n / 2 + 1 terms per MSM (n terms in step 1)
    assert 4 * native_lib.IPA_MAX_PROVERS <= native_lib.FIXED_MAX_MSMS and native_lib.IPA_MAX_N <= native_lib.FIXED_MAX_TERMS
