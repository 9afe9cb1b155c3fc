"""The device prover of the grand-product argument, the parts that run without a GPU: the element formulas, the completion of the IPA's
blinders and the term schedule k_gprod_step runs (cg1_gprod_emulate is compiled from csrc/gprod_rounds.h, the header the kernel includes)
against the reference's GrandProductProof.new as recorded in tests/golden/grand_product_device_vectors.json -- vec_c, r_p, inner_prod,
vec_d (in full or by its digest) and the completed blinders for every case, and for the small cases every term list evaluated with the CPU oracle against B and the
points IPA.new received or produced -- plus the refusals and the symbol lists."""
import ctypes
import hashlib
import json
import os
import re

import pytest

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = O.R
GPROD = ["cg1_gprod_proof_bytes", "cg1_gprod_prove_device", "cg1_gprod_emulate"]
SHAPES = [(1, 3), (2, 2), (6, 2), (4, 4), (28, 4), (124, 4), (508, 4)]


@pytest.fixture(scope="module")
def cases():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "grand_product_device_vectors.json")))["cases"]


def s32(values):
    return b"".join(v.to_bytes(32, "little") for v in values)


def ints(raw, n):
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(n)]


def le(h):
    return int.from_bytes(bytes.fromhex(h), "little")


def inputs_of(case):
    """The emulator's scalar inputs as Python ints (mutable: the refusal tests edit them)."""
    g = lambda k: [le(h) for h in case[k]]
    return dict(ell=case["ell"], nb=case["n_blinders"], gres=le(case["gprod_result"]), b=g("vec_b") + g("vec_b_blinders"), cbl=g("vec_c_blinders"),
                r=g("ipa_r"), z=g("ipa_z_head"), alpha=le(case["gprod_alpha"]), beta=le(case["gprod_beta"]))


def emulate(N, inp, want=0):
    """-> (rc, status, dict of outputs).  Table layout of the tests: crs_G_vec | crs_H_vec at 0 .. n-1, crs_U at n."""
    ell, nb = inp["ell"], inp["nb"]
    n = ell + nb
    gi = (ctypes.c_uint32 * max(1, n))(*range(n))
    state, two = ctypes.create_string_buffer(32 * 4 * max(1, n)), ctypes.create_string_buffer(64)
    tb, sc, offs, st = (ctypes.c_uint32 * (5 * max(1, n)))(), ctypes.create_string_buffer(32 * 5 * max(1, n)), (ctypes.c_uint32 * 6)(), ctypes.c_uint32(0xffffffff)
    rc = N.cg1_gprod_emulate(ell, nb, s32([inp["gres"]]), s32(inp["b"]), s32(inp["cbl"]), s32(inp["r"]), s32(inp["z"]), s32([inp["alpha"]]), s32([inp["beta"]]),
                             gi, state, two, tb, sc, offs, ctypes.byref(st))
    assert rc == want, (rc, want, hex(st.value))
    raw = state.raw
    out = dict(c=ints(raw, n), d=ints(raw[32 * n:], n), kgp=ints(raw[64 * n:], n), z=ints(raw[96 * n:], n), r_p=ints(two.raw, 2)[0], inner_prod=ints(two.raw, 2)[1],
               tb=list(tb), sc=ints(sc.raw, 5 * n), offs=list(offs))
    return rc, st.value, out


def test_fixture_shape(cases):
    assert [(c["ell"], c["n_blinders"]) for c in cases] == SHAPES
    for c in cases:
        n = c["ell"] + c["n_blinders"]
        lg = n.bit_length() - 1
        assert len(c["proof"]) // 2 == 48 + 32 + (2 + 4 * lg) * 48 + 64 and len(c["ipa_gammas"]) == lg
        assert len(c["vec_c_blinders"]) == c["n_blinders"] and len(c["ipa_r"]) == n and len(c["ipa_z_head"]) == n - 2
        assert len(c["ipa_z_tail"]) == 2 and ("crs_G_vec" in c) == ("vec_d" in c) == (n <= 32)      # beyond: bases from the seed, vec_d as its digest
        assert c["proof"][:96] == c["ipa_C"]                            # GrandProductProof.to_bytes starts with the C that IPA.new received


def test_scalars_every_case(native_lib, cases):
    """vec_c is the prefix products; r_p, inner_prod, vec_d and the completed blinders are the reference's; its two relations hold."""
    for case in cases:
        inp = inputs_of(case)
        ell, nb = inp["ell"], inp["nb"]
        n = ell + nb
        _, st, out = emulate(native_lib, inp)
        assert st == 0
        pre, want_c = 1, []
        for i in range(ell):
            want_c.append(pre)
            pre = pre * inp["b"][i] % R
        assert pre == inp["gres"] and out["c"] == want_c + inp["cbl"], (ell, nb)
        proof = bytes.fromhex(case["proof"])
        assert out["r_p"] == int.from_bytes(proof[48:80], "little")
        assert out["inner_prod"] == le(case["ipa_z"])
        assert hashlib.sha256(s32(out["d"])).hexdigest() == case["vec_d_sha256"], (ell, nb)
        assert "vec_d" not in case or out["d"] == [le(h) for h in case["vec_d"]], (ell, nb)
        binv = pow(inp["beta"], -1, R)
        assert out["kgp"] == [pow(binv, i + 1, R) for i in range(ell)] + [pow(binv, ell + 1, R)] * nb
        assert out["z"] == [le(h) for h in case["ipa_z_head"] + case["ipa_z_tail"]], (ell, nb)
        dot = lambda a, b: sum(x * y for x, y in zip(a, b)) % R
        assert (dot(inp["r"], out["d"]) + dot(out["z"], out["c"])) % R == 0 and dot(inp["r"], out["z"]) == 0      # ipa.py:45-46
        assert dot(out["c"], out["d"]) == out["inner_prod"]                                                       # grand_prod.py:103
        assert out["offs"] == [q * n for q in range(6)] and all(v < R for v in out["sc"]) and all(t < n for t in out["tb"])


def evaluate(bases, tb, sc, lo, hi):
    acc = None
    for i in range(lo, hi):
        assert tb[i] >> 31 == 0                                          # no negated base in this schedule
        acc = O.g1_add(acc, O.g1_mul(bases[tb[i]], sc[i]))
    return O.g1_compress(acc)


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_term_lists_give_the_reference_points(native_lib, cases, which):
    """The cases with n <= 8: the five term lists, evaluated by the oracle over the fixture's bases, give B, C, D, B_c, B_d."""
    case = cases[which]
    n = case["ell"] + case["n_blinders"]
    assert n in (4, 8)
    dec = lambda h: O.g1_decompress(bytes.fromhex(h))
    bases = [dec(h) for h in case["crs_G_vec"]] + [dec(h) for h in case["crs_H_vec"]]
    _, _, out = emulate(native_lib, inputs_of(case))
    got = [evaluate(bases, out["tb"], out["sc"], q * n, (q + 1) * n).hex() for q in range(5)]
    proof = case["proof"]
    assert got == [case["B"], case["ipa_C"], case["ipa_D"], proof[160:256], proof[256:352]]


def test_refusals(native_lib, cases):
    N = native_lib
    base = inputs_of(cases[3])                                           # (4, 4)
    n = 8
    edit = lambda **kw: {**{k: (list(v) if isinstance(v, list) else v) for k, v in base.items()}, **kw}
    for bad in (R, R + 5, (1 << 256) - 1):                               # a scalar >= r is refused, never reduced
        for key in ("gres", "alpha", "beta"):
            emulate(N, edit(**{key: bad}), want=N.ERR_ENCODING)
        for key, at in (("b", 0), ("b", n - 1), ("cbl", 1), ("r", 3), ("z", n - 3)):
            v = list(base[key])
            v[at] = bad
            emulate(N, edit(**{key: v}), want=N.ERR_ENCODING)
    _, st, _ = emulate(N, edit(beta=0), want=N.ERR_ARG)                  # beta = 0 has no inverse
    assert st == N.GPROD_ZERO_BETA
    cbl = list(base["cbl"])
    cbl[-2] = 0                                                          # c[n-2] = 0: the first denominator
    _, st, _ = emulate(N, edit(cbl=cbl), want=N.ERR_ARG)
    assert st & N.GPROD_ZERO_C
    r = list(base["r"])                                                  # the second denominator: r[n-1] = r[n-2] c[n-1] / c[n-2]
    r[-1] = r[-2] * base["cbl"][-1] * pow(base["cbl"][-2], -1, R) % R
    _, st, _ = emulate(N, edit(r=r), want=N.ERR_ARG)
    assert st == N.GPROD_ZERO_DENOMINATOR
    _, st, _ = emulate(N, edit(gres=(base["gres"] + 1) % R), want=N.ERR_ARG)
    assert st == N.GPROD_BAD_PRODUCT
    b = list(base["b"])
    b[1] = (b[1] + 1) % R
    _, st, _ = emulate(N, edit(b=b), want=N.ERR_ARG)
    assert st == N.GPROD_BAD_PRODUCT
    for ell, nb in ((0, 4), (0, 8), (7, 1), (8, 0), (3, 3), (5, 2), (1, 2), (4092, 4), (2, 4)):      # bad shapes
        pad = lambda v, k: (list(v) + [1] * k)[:k]
        emulate(N, dict(base, ell=ell, nb=nb, b=pad(base["b"], ell + nb), cbl=pad(base["cbl"], nb), r=pad(base["r"], ell + nb), z=pad(base["z"], max(0, ell + nb - 2))),
                want=N.ERR_ARG)
    _, st, out = emulate(N, base)                                        # and the inputs are still good
    assert st == 0 and out["z"] == [le(h) for h in cases[3]["ipa_z_head"] + cases[3]["ipa_z_tail"]]


def test_proof_bytes(native_lib):
    N = native_lib
    assert N.cg1_gprod_proof_bytes(124, 4) == 1584 and N.cg1_gprod_proof_bytes(1, 3) == 624 and N.cg1_gprod_proof_bytes(508, 4) == 1968
    assert N.cg1_gprod_proof_bytes(124, 4) == 48 + 32 + N.cg1_ipa_proof_bytes(128)
    for ell, nb in ((0, 4), (4, 0), (7, 1), (3, 3), (5, 2), (1, 2), (0, 0)):
        assert N.cg1_gprod_proof_bytes(ell, nb) == 0, (ell, nb)


def test_symbol_lists_agree(native_lib):
    src = open(os.path.join(ROOT, "include", "curdle_g1.h")).read()
    stripped = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cg1_[a-z0-9_]+)\s*\(", stripped))
    lib = ctypes.CDLL(native_lib.LIB_PATH)
    for name in GPROD:
        assert name in declared and hasattr(lib, name) and name in native_lib.EXPORTED_SYMBOLS and callable(getattr(native_lib, name)), name
    assert sorted(native_lib.EXPORTED_SYMBOLS) == sorted(declared)
    for name in ("BAD_COMMITMENT", "BAD_PRODUCT", "ZERO_BETA", "ZERO_C", "ZERO_DENOMINATOR"):
        assert re.search(r"#define\s+CG1_GPROD_%s\s+0x%x\b" % (name, getattr(native_lib, "GPROD_" + name)), stripped), name
    # 4 MSMs per prover per launch in the rounds, 3 of n terms before them
    assert 4 * native_lib.IPA_MAX_PROVERS <= native_lib.FIXED_MAX_MSMS and native_lib.IPA_MAX_N <= native_lib.FIXED_MAX_TERMS
