"""The device prover of the same-MSM argument, the parts that run without a GPU: the scalar schedule and the fold k_smsm_step runs
(cg1_same_msm_round_emulate is compiled from csrc/same_msm_rounds.h, the header the kernel includes) against the reference's
SameMSMProof.new as recorded in tests/golden/same_msm_device_vectors.json -- x_final for every case, and for the small cases every term
list evaluated with the CPU oracle against the proof's points -- plus the refusals and the symbol lists."""
import ctypes
import json
import os
import re

import pytest

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = O.R
SMSM = ["cg1_same_msm_proof_bytes", "cg1_same_msm_prove_device", "cg1_same_msm_round_emulate"]


@pytest.fixture(scope="module")
def cases():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "same_msm_device_vectors.json")))["cases"]


def s32(values):
    return b"".join(v.to_bytes(32, "little") for v in values)


def ints(raw, n):
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(n)]


def le(h):
    return int.from_bytes(bytes.fromhex(h), "little")


class Emu:
    """One prover's state driven through cg1_same_msm_round_emulate."""

    def __init__(self, N, case):
        n = self.n0 = self.len = case["n"]
        self.N = N
        self.x = ctypes.create_string_buffer(s32([le(h) for h in case["vec_x"]]), 32 * n)
        self.k = ctypes.create_string_buffer(s32([1] * n), 32 * n)
        self.r = s32([le(h) for h in case["vec_r"]])
        self.gi = (ctypes.c_uint32 * n)(*range(100, 100 + n))            # the fixed table of the tests: G[j] at 100 + j

    def call(self, op, challenge=None, want=0):
        n = self.n0
        nt, nm = 3 * n, (3 if op == 0 else 6)
        tb, sc, offs = (ctypes.c_uint32 * nt)(), ctypes.create_string_buffer(32 * nt), (ctypes.c_uint32 * (nm + 1))()
        rc = self.N.cg1_same_msm_round_emulate(op, n, self.len, self.x, self.k, None if challenge is None else s32([challenge]), self.r, self.gi, tb, sc, offs)
        assert rc == want, (op, rc)
        if op == 2 and challenge is not None and rc == 0:
            self.len //= 2
        return list(tb), ints(sc.raw, nt), list(offs)

    def vector(self):
        return ints(self.x.raw, self.len)


def proof_fields(case):
    n, raw = case["n"], bytes.fromhex(case["proof"])
    lg = n.bit_length() - 1
    pts = [raw[48 * j: 48 * j + 48] for j in range(3 + 6 * lg)]
    vec = lambda q: pts[3 + q * lg: 3 + (q + 1) * lg]
    return dict(B=pts[:3], rounds=[[vec(q)[k] for q in range(6)] for k in range(lg)], x_final=int.from_bytes(raw[-32:], "little"))


def oracle_msm(points, scalars):
    acc = None
    for p, s in zip(points, scalars):
        acc = O.g1_add(acc, O.g1_mul(p, s))
    return O.g1_compress(acc)


def test_fixture_shape(cases):
    assert [(c["n"], c["shape"]) for c in cases] == [(2, "random"), (8, "random"), (32, "random"), (128, "random"), (8, "shuffle"), (128, "shuffle")]
    inf = (b"\xc0" + bytes(47)).hex()
    for c in cases:
        n, lg = c["n"], c["n"].bit_length() - 1
        assert len(c["proof"]) // 2 == (3 + 6 * lg) * 48 + 32 and len(c["gammas"]) == lg
        assert len(c["crs_G_vec"]) == len(c["vec_T"]) == len(c["vec_U"]) == len(c["vec_x"]) == len(c["vec_r"]) == n
        if c["shape"] == "shuffle":                                      # curdleproofs.py:124-136, and H is a CRS base
            H = c["crs_G_vec"][0]
            assert c["vec_T"][-4:] == [inf, inf, H, inf] and c["vec_U"][-4:] == [inf, inf, inf, H]
    for c in cases:
        if c["n"] > 8:
            continue
        x = [le(h) for h in c["vec_x"]]                                  # A, Z_t, Z_u are consistent with x
        for vec, res in (("crs_G_vec", "A"), ("vec_T", "Z_t"), ("vec_U", "Z_u")):
            assert oracle_msm([O.g1_decompress(bytes.fromhex(h)) for h in c[vec]], x).hex() == c[res], (c["n"], res)


def test_x_final_every_case(native_lib, cases):
    """Blinding with the recorded alpha and folding with the recorded gammas gives the proof's x_final (Fr only)."""
    for case in cases:
        e = Emu(native_lib, case)
        e.call(1, le(case["alpha"]))
        alpha = le(case["alpha"])
        assert e.vector() == [(le(r) + alpha * le(x)) % R for r, x in zip(case["vec_r"], case["vec_x"])]
        for g in case["gammas"]:
            e.call(2, le(g))
        assert e.len == 1 and e.vector() == [proof_fields(case)["x_final"]], (case["n"], case["shape"])


@pytest.mark.parametrize("which", [0, 1, 4])
def test_term_lists_give_the_reference_points(native_lib, cases, which):
    """n = 2 and both n = 8 cases: every launch's term lists, evaluated by the oracle over the fixture's bases."""
    case = cases[which]
    n = case["n"]
    assert n in (2, 8)
    dec = lambda h: O.g1_decompress(bytes.fromhex(h))
    G, T, U = ([dec(h) for h in case[k]] for k in ("crs_G_vec", "vec_T", "vec_U"))
    TU = T + U

    def evaluate(tb, sc, lo, hi, fixed):
        assert all(t >> 31 == 0 for t in tb[lo:hi])                      # no negated base in this schedule
        if fixed:
            assert all(100 <= t < 100 + n for t in tb[lo:hi])
            return oracle_msm([G[t - 100] for t in tb[lo:hi]], sc[lo:hi])
        assert all(t < 2 * n for t in tb[lo:hi])
        return oracle_msm([TU[t] for t in tb[lo:hi]], sc[lo:hi])

    want = proof_fields(case)
    e = Emu(native_lib, case)
    tb, sc, offs = e.call(0)
    assert offs == [0, n, 2 * n, 3 * n]
    assert [evaluate(tb, sc, offs[j], offs[j + 1], j == 0) for j in range(3)] == want["B"]
    assert tb[n: 2 * n] == list(range(n)) and tb[2 * n:] == list(range(n, 2 * n))      # B_t over T, B_u over U
    e.call(1, le(case["alpha"]))
    h = n // 2
    for k, g in enumerate(case["gammas"]):
        tb, sc, offs = e.call(2, le(g))
        assert offs == [j * h for j in range(7)]
        assert all(v < R for v in sc)
        got = [evaluate(tb, sc, offs[j], offs[j + 1], j % 3 == 0) for j in range(6)]
        assert got == want["rounds"][k], (n, k)
        for j in (1, 4):                                                 # T lists index T, U lists the same positions of U
            assert all(t < n for t in tb[offs[j]: offs[j + 1]]) and [t + n for t in tb[offs[j]: offs[j + 1]]] == tb[offs[j + 1]: offs[j + 2]]


def test_terms_without_a_fold_leave_the_state(native_lib, cases):
    e = Emu(native_lib, cases[1])
    e.call(1, le(cases[1]["alpha"]))
    before = (e.x.raw, e.k.raw)
    a = e.call(2)
    assert (e.x.raw, e.k.raw) == before and e.len == 8
    assert e.call(2) == a


def test_refusals(native_lib, cases):
    N = native_lib
    assert N.cg1_same_msm_proof_bytes(2) == 464 and N.cg1_same_msm_proof_bytes(8) == 1040 and N.cg1_same_msm_proof_bytes(128) == 2192
    for bad in (0, 1, 3, 6):
        assert N.cg1_same_msm_proof_bytes(bad) == 0
    e = Emu(N, cases[1])
    for bad in (R, R + 5, (1 << 256) - 1):                               # a scalar >= r is refused, never reduced
        e.call(1, bad, want=N.ERR_ENCODING)
        keep = e.x.raw
        e.x = ctypes.create_string_buffer(s32([bad]) + keep[32:], len(keep))
        before = e.k.raw
        e.call(2, 5, want=N.ERR_ENCODING)
        assert e.k.raw == before
        e.x = ctypes.create_string_buffer(keep, len(keep))
    before = (e.x.raw, e.k.raw)
    e.call(2, 0, want=N.ERR_ARG)                                         # gamma = 0 has no inverse
    assert (e.x.raw, e.k.raw) == before
    for n0, ln in ((6, 6), (1, 1), (8, 3), (8, 16), (12, 4)):            # not a power of two, below 2, longer than n0
        e2 = Emu(N, cases[1])
        e2.n0, e2.len = n0, ln
        e2.call(2, 5, want=N.ERR_ARG)
    e.call(1, le(cases[1]["alpha"]))                                     # and the state is still usable
    for g in cases[1]["gammas"]:
        e.call(2, le(g))
    assert e.vector() == [proof_fields(cases[1])["x_final"]]


def test_symbol_lists_agree(native_lib):
    src = open(os.path.join(ROOT, "include", "curdle_g1.h")).read()
    stripped = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cg1_[a-z0-9_]+)\s*\(", stripped))
    lib = ctypes.CDLL(native_lib.LIB_PATH)
    for name in SMSM:
        assert name in declared and hasattr(lib, name) and name in native_lib.EXPORTED_SYMBOLS and callable(getattr(native_lib, name)), name
    assert sorted(native_lib.EXPORTED_SYMBOLS) == sorted(declared)
    for macro, value in (("CG1_SAME_MSM_MAX_N", native_lib.SAME_MSM_MAX_N), ("CG1_SAME_MSM_MAX_PROVERS", native_lib.SAME_MSM_MAX_PROVERS)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), stripped), macro
    # per launch: 2 MSMs per prover over the fixed table, 4 over the light table, n terms at most (step B)
    assert 2 * native_lib.SAME_MSM_MAX_PROVERS <= native_lib.FIXED_MAX_MSMS and 4 * native_lib.SAME_MSM_MAX_PROVERS <= native_lib.LIGHT_MAX_MSMS
    assert native_lib.SAME_MSM_MAX_N <= native_lib.FIXED_MAX_TERMS and 2 * native_lib.SAME_MSM_MAX_N <= native_lib.LIGHT_MAX_BASES
