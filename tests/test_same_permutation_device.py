"""The device prover of the same-permutation argument, the parts that run without a GPU: the host transcript head, the polynomial factors,
their product and the term schedule k_same_perm_begin runs (cg1_same_perm_emulate is compiled from csrc/same_perm_rounds.h, the header the
kernel includes) against the reference's SamePermutationProof.new as recorded in tests/golden/same_permutation_device_vectors.json --
same_perm_alpha, same_perm_beta, vec_b (in full or by its digest), vec_b_blinders and gprod_result for every case, and for the small cases
the four term lists evaluated with the CPU oracle against A, M, the B the reference computed and the proof's C -- plus the refusals and the
symbol lists."""
import ctypes
import hashlib
import json
import os
import re

import pytest

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = O.R
SAME_PERM = ["cg1_same_perm_proof_bytes", "cg1_same_perm_prove_device", "cg1_same_perm_emulate"]
SHAPES = [(1, 3), (2, 2), (6, 2), (4, 4), (28, 4), (124, 4), (508, 4)]


@pytest.fixture(scope="module")
def cases():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "same_permutation_device_vectors.json")))["cases"]


def s32(values):
    return b"".join(v.to_bytes(32, "little") for v in values)


def ints(raw, n):
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(n)]


def le(h):
    return int.from_bytes(bytes.fromhex(h), "little")


def start_state(N, case):
    st = ctypes.create_string_buffer(N.MERLIN_STATE_BYTES)
    label, plabel, prefix = case["label"].encode(), case["prefix_label"].encode(), bytes.fromhex(case["prefix"])
    N.cg1_merlin_init(st, label, len(label))
    N.cg1_merlin_append(st, plabel, len(plabel), prefix, len(prefix))
    return st.raw


def inputs_of(case):
    """The emulator's inputs, scalars as Python ints (mutable: the refusal tests edit them)."""
    g = lambda k: [le(h) for h in case[k]]
    return dict(ell=case["ell"], nb=case["n_blinders"], A=bytes.fromhex(case["A"]), M=bytes.fromhex(case["M"]), a=g("vec_a"), perm=list(case["permutation"]),
                abl=g("vec_a_blinders"), mbl=g("vec_m_blinders"), cbl=g("vec_c_blinders"))


def emulate(N, case, inp, want=0):
    """-> (status, dict of outputs).  Table layout of the tests: crs_G_vec | crs_H_vec at 0 .. n-1, crs_U at n."""
    ell, nb = inp["ell"], inp["nb"]
    n = ell + nb
    m = max(1, n)
    start = start_state(N, case)
    state = ctypes.create_string_buffer(start, N.MERLIN_STATE_BYTES)
    gi = (ctypes.c_uint32 * m)(*range(n))
    perm = (ctypes.c_uint32 * max(1, len(inp["perm"])))(*inp["perm"])
    ab, b, gres = ctypes.create_string_buffer(64), ctypes.create_string_buffer(32 * m), ctypes.create_string_buffer(32)
    tb, sc, offs, st = (ctypes.c_uint32 * (4 * m))(), ctypes.create_string_buffer(32 * 4 * m), (ctypes.c_uint32 * 5)(), ctypes.c_uint32(0xffffffff)
    rc = N.cg1_same_perm_emulate(ell, nb, state, inp["A"], inp["M"], s32(inp["a"]), perm, s32(inp["abl"]), s32(inp["mbl"]), s32(inp["cbl"]), gi, ab, b, gres, tb, sc,
                                 offs, ctypes.byref(st))
    assert rc == want, (rc, want)
    if rc != N.OK:
        assert state.raw == start                                        # a refused call leaves the transcript alone
        return st.value, None
    return st.value, dict(alpha=ints(ab.raw, 2)[0], beta=ints(ab.raw, 2)[1], b=ints(b.raw, n), gres=ints(gres.raw, 1)[0], tb=list(tb), sc=ints(sc.raw, 4 * n),
                          offs=list(offs), state=state.raw, start=start)


def test_fixture_shape(cases):
    assert [(c["ell"], c["n_blinders"]) for c in cases] == SHAPES
    kinds = [c["permutation_kind"] for c in cases]
    assert "identity" in kinds and "reversed" in kinds
    for c in cases:
        ell, nb = c["ell"], c["n_blinders"]
        n = ell + nb
        lg = n.bit_length() - 1
        assert len(c["proof"]) // 2 == 48 + 48 + 32 + (2 + 4 * lg) * 48 + 64 and len(c["ipa_gammas"]) == lg
        assert len(c["vec_a"]) == len(c["permutation"]) == ell and sorted(c["permutation"]) == list(range(ell))
        assert len(c["vec_a_blinders"]) == len(c["vec_m_blinders"]) == len(c["vec_c_blinders"]) == len(c["vec_b_blinders"]) == nb
        assert len(c["ipa_r"]) == n and len(c["ipa_z_head"]) == n - 2
        assert ("crs_G_vec" in c) == ("vec_b" in c) == (n <= 32)          # beyond: bases from the seed, vec_b as its digest
        assert c["proof"][:96] == c["B"]                                  # SamePermutationProof.to_bytes starts with B
        if c["permutation_kind"] == "identity":
            assert c["permutation"] == list(range(ell))
        if c["permutation_kind"] == "reversed":
            assert c["permutation"] == list(range(ell))[::-1]
    big = cases[5]
    assert (big["ell"], big["n_blinders"]) == (124, 4) and [le(h) for h in big["vec_a_blinders"][2:]] == [0, 0]


def test_scalars_every_case(native_lib, cases):
    """alpha and beta come out of the host transcript; vec_b, vec_b_blinders and gprod_result are what GrandProductProof.new received."""
    for case in cases:
        inp = inputs_of(case)
        ell, nb = inp["ell"], inp["nb"]
        n = ell + nb
        st, out = emulate(native_lib, case, inp)
        assert st == 0 and out["state"] != out["start"]
        assert out["alpha"] == le(case["same_perm_alpha"]) and out["beta"] == le(case["same_perm_beta"]), (ell, nb)
        assert hashlib.sha256(s32(out["b"][:ell])).hexdigest() == case["vec_b_sha256"], (ell, nb)
        assert "vec_b" not in case or out["b"][:ell] == [le(h) for h in case["vec_b"]], (ell, nb)
        assert out["b"][ell:] == [le(h) for h in case["vec_b_blinders"]], (ell, nb)
        assert out["gres"] == le(case["gprod_result"]), (ell, nb)
        want = [(inp["a"][m] + m * out["alpha"] + out["beta"]) % R for m in inp["perm"]]      # same_perm.py:49-51
        assert out["b"][:ell] == want
        assert out["offs"] == [q * n for q in range(5)] and all(v < R for v in out["sc"]) and all(t < n for t in out["tb"])
        # the scalar lists: vec_a o perm | a blinders, perm | m blinders, b | b blinders, prefix products | c blinders
        pre, prods = 1, []
        for x in want:
            prods.append(pre)
            pre = pre * x % R
        assert out["sc"] == [inp["a"][m] for m in inp["perm"]] + inp["abl"] + inp["perm"] + inp["mbl"] + out["b"] + prods + inp["cbl"]


def evaluate(bases, tb, sc, lo, hi):
    acc = None
    for i in range(lo, hi):
        assert tb[i] >> 31 == 0                                          # no negated base in this schedule
        acc = O.g1_add(acc, O.g1_mul(bases[tb[i]], sc[i]))
    return O.g1_compress(acc)


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_term_lists_give_the_reference_points(native_lib, cases, which):
    """The cases with n <= 8: the four term lists, evaluated by the oracle over the fixture's bases, give A, M, the reference's B, C."""
    case = cases[which]
    n = case["ell"] + case["n_blinders"]
    assert n in (4, 8)
    dec = lambda h: O.g1_decompress(bytes.fromhex(h))
    bases = [dec(h) for h in case["crs_G_vec"]] + [dec(h) for h in case["crs_H_vec"]]
    _, out = emulate(native_lib, case, inputs_of(case))
    got = [evaluate(bases, out["tb"], out["sc"], q * n, (q + 1) * n).hex() for q in range(4)]
    assert got == [case["A"], case["M"], case["B"], case["proof"][96:192]]


def test_refusals(native_lib, cases):
    N = native_lib
    case = cases[3]                                                      # (4, 4)
    base = inputs_of(case)
    edit = lambda **kw: {**{k: (list(v) if isinstance(v, list) else v) for k, v in base.items()}, **kw}
    for bad in (R, R + 5, (1 << 256) - 1):                               # a scalar >= r is refused, never reduced
        for key, at in (("a", 0), ("a", 3), ("abl", 1), ("mbl", 3), ("cbl", 2)):
            v = list(base[key])
            v[at] = bad
            emulate(N, case, edit(**{key: v}), want=N.ERR_ENCODING)
    for at, m in ((0, 4), (3, 4), (2, 7), (1, 0xffffffff)):              # perm entry >= ell: the reference's get_permutation raises IndexError
        perm = list(base["perm"])
        perm[at] = m
        emulate(N, case, edit(perm=perm), want=N.ERR_ARG)
    for ell, nb in ((0, 4), (0, 8), (7, 1), (8, 0), (3, 3), (5, 2), (1, 2), (4092, 4), (2, 4)):      # bad shapes
        pad = lambda v, k: (list(v) + [1] * k)[:k]
        emulate(N, case, dict(base, ell=ell, nb=nb, a=pad(base["a"], ell), perm=[0] * ell, abl=pad(base["abl"], nb), mbl=pad(base["mbl"], nb), cbl=pad(base["cbl"], nb)),
                want=N.ERR_ARG)
    flagless = bytes([base["A"][0] & 0x7F]) + base["A"][1:]              # an undecodable A, an undecodable M
    emulate(N, case, edit(A=flagless), want=N.ERR_ENCODING)
    emulate(N, case, edit(M=flagless), want=N.ERR_ENCODING)
    x_not_on_curve = next(bytes([0x80]) + bytes(46) + bytes([x]) for x in range(1, 40) if N.cg1_validate_compressed(bytes([0x80]) + bytes(46) + bytes([x]), None) != N.OK)
    emulate(N, case, edit(A=x_not_on_curve), want=N.ERR_NOT_ON_CURVE)
    perm = [1, 1, 3, 1]                                                  # not a bijection: accepted, as by the reference
    st, out = emulate(N, case, edit(perm=perm))
    assert st == 0 and out["b"][:4] == [(base["a"][m] + m * out["alpha"] + out["beta"]) % R for m in perm]
    st, out = emulate(N, case, base)                                     # and the inputs are still good
    assert st == 0 and out["gres"] == le(case["gprod_result"])


def test_proof_bytes(native_lib):
    N = native_lib
    assert N.cg1_same_perm_proof_bytes(124, 4) == 1632 and N.cg1_same_perm_proof_bytes(1, 3) == 672 and N.cg1_same_perm_proof_bytes(508, 4) == 2016
    assert N.cg1_same_perm_proof_bytes(124, 4) == 48 + N.cg1_gprod_proof_bytes(124, 4)
    for ell, nb in ((0, 4), (4, 0), (7, 1), (3, 3), (5, 2), (1, 2), (0, 0)):
        assert N.cg1_same_perm_proof_bytes(ell, nb) == 0, (ell, nb)


def test_symbol_lists_agree(native_lib):
    src = open(os.path.join(ROOT, "include", "curdle_g1.h")).read()
    stripped = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cg1_[a-z0-9_]+)\s*\(", stripped))
    lib = ctypes.CDLL(native_lib.LIB_PATH)
    for name in SAME_PERM:
        assert name in declared and hasattr(lib, name) and name in native_lib.EXPORTED_SYMBOLS and callable(getattr(native_lib, name)), name
    assert sorted(native_lib.EXPORTED_SYMBOLS) == sorted(declared)
    values = {}
    for name in ("BAD_A", "BAD_M"):
        values[name] = getattr(native_lib, "SAME_PERM_" + name)
        assert re.search(r"#define\s+CG1_SAME_PERM_%s\s+0x%x\b" % (name, values[name]), stripped), name
    gprod = [getattr(native_lib, "GPROD_" + k) for k in ("BAD_COMMITMENT", "BAD_PRODUCT", "ZERO_BETA", "ZERO_C", "ZERO_DENOMINATOR")]
    assert values == {"BAD_A": 0x2000, "BAD_M": 0x4000} and min(values.values()) > max(gprod)      # above CG1_GPROD_*
    # 4 MSMs of n terms per prover in the first launch, as in the rounds
    assert 4 * native_lib.IPA_MAX_PROVERS <= native_lib.FIXED_MAX_MSMS and native_lib.IPA_MAX_N <= native_lib.FIXED_MAX_TERMS
