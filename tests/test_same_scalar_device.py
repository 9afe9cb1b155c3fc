"""The device prover of the shuffle prover's same-scalar block, the parts that run without a GPU: the term schedule and the responses
k_sscalar_step runs (cg1_same_scalar_emulate is compiled from csrc/same_scalar_rounds.h, the header the kernel includes) against the
reference's own run of curdleproofs.py:92-116 as recorded in tests/golden/same_scalar_device_vectors.json -- the schedule recomputed in
Python ints for every case, alpha, z_k, z_t, z_u and the final transcript state for every case, and for the small cases every term list
evaluated with the CPU oracle against the proof's points -- plus the refusals and the symbol lists."""
import ctypes
import json
import os
import re

import pytest

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = O.R
SSCALAR = ["cg1_same_scalar_proof_bytes", "cg1_same_scalar_prove_device", "cg1_same_scalar_emulate"]
ELLS = [1, 2, 5, 8, 28, 124]
# the proof's 48-byte slots in the transcript's order R, S, T.T_1, T.T_2, U.T_1, U.T_2, A.T_1, A.T_2, B.T_1, B.T_2:
# cm_T | cm_U | R | S | cm_A | cm_B | z_k | z_t | z_u
SLOTS = [4, 5, 0, 1, 2, 3, 6, 7, 8, 9]


@pytest.fixture(scope="module")
def cases():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "same_scalar_device_vectors.json")))["cases"]


def s32(values):
    return b"".join(v.to_bytes(32, "little") for v in values)


def ints(raw, n):
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(n)]


def le(h):
    return int.from_bytes(bytes.fromhex(h), "little")


def blinders(case):
    return [le(case[key]) for key in ("r_t", "r_u", "r_a", "r_b", "r_k")]


def encodings(case):
    """The ten encodings in the transcript's order."""
    raw = bytes.fromhex(case["proof"])
    return b"".join(raw[48 * s: 48 * s + 48] for s in SLOTS)


def start_state(N, case):
    """The 208-byte transcript state where the block finds it."""
    st = ctypes.create_string_buffer(208)
    label = case["label"].encode()
    N.cg1_merlin_init(st, label, len(label))
    pl, msg = case["prefix_label"].encode(), bytes.fromhex(case["prefix"])
    N.cg1_merlin_append(st, pl, len(pl), msg, len(msg))
    return st


def emulate(N, ell, vec_a, k, bl, enc=None, state=None, want=0):
    nt = 6 * ell + 8
    tb, sc, offs = (ctypes.c_uint32 * max(1, nt))(), ctypes.create_string_buffer(32 * max(1, nt)), (ctypes.c_uint32 * 11)()
    alpha, z = ctypes.create_string_buffer(32), ctypes.create_string_buffer(96)
    rc = N.cg1_same_scalar_emulate(ell, s32(vec_a), s32([k]), s32(bl), enc, state, tb, sc, offs, alpha, z)
    assert rc == want, rc
    return list(tb), ints(sc.raw, nt), list(offs), int.from_bytes(alpha.raw, "little"), ints(z.raw, 3)


def schedule(ell, a, k, bl):
    """The table of the ten MSMs in Python ints: per MSM a list of (base index, scalar); G_t, G_u, H at 0, 1, 2, R_j at 3 + j, S_j at
    3 + ell + j."""
    r_t, r_u, r_a, r_b, r_k = bl
    Rj, Sj = [3 + j for j in range(ell)], [3 + ell + j for j in range(ell)]
    ka, rka = [k * x % R for x in a], [r_k * x % R for x in a]
    return [list(zip(Rj, a)), list(zip(Sj, a)),
            [(0, r_t)], list(zip(Rj, ka)) + [(2, r_t)], [(1, r_u)], list(zip(Sj, ka)) + [(2, r_u)],
            [(0, r_a)], list(zip(Rj, rka)) + [(2, r_a)], [(1, r_b)], list(zip(Sj, rka)) + [(2, r_b)]]


def test_fixture_shape(cases):
    assert [c["ell"] for c in cases] == ELLS
    for c in cases:
        assert len(c["proof"]) == 2 * 576 and len(c["vec_a"]) == c["ell"]
        assert ("vec_R" in c) == (c["ell"] <= 32)
        if c["ell"] <= 32:
            assert len(c["vec_R"]) == len(c["vec_S"]) == c["ell"]


@pytest.mark.parametrize("which", range(len(ELLS)))
def test_schedule_alpha_and_responses_every_case(native_lib, cases, which):
    N, c = native_lib, cases[which]
    ell, a, k, bl = c["ell"], [le(h) for h in c["vec_a"]], le(c["k"]), blinders(c)
    st = start_state(N, c)
    tb, sc, offs, alpha, z = emulate(N, ell, a, k, bl, encodings(c), st)
    want = schedule(ell, a, k, bl)
    lens = [ell, ell, 1, ell + 1, 1, ell + 1, 1, ell + 1, 1, ell + 1]
    assert [len(m) for m in want] == lens
    assert offs == [sum(lens[:q]) for q in range(11)] and offs[10] == 6 * ell + 8
    for q in range(10):
        assert list(zip(tb[offs[q]: offs[q + 1]], sc[offs[q]: offs[q + 1]])) == want[q], (ell, q)
    assert all(v < R for v in sc) and all(t >> 31 == 0 for t in tb)
    # ---- alpha, z_k, z_t, z_u, and the state afterwards
    assert alpha == le(c["alpha"])
    r_t, r_u, r_a, r_b, r_k = bl
    assert z == [(r_k + k * alpha) % R, (r_a + r_t * alpha) % R, (r_b + r_u * alpha) % R]
    assert s32(z) == bytes.fromhex(c["proof"])[480:]
    after = ctypes.create_string_buffer(32)
    N.cg1_merlin_challenge_scalar(st, b"after", 5, after)
    assert after.raw.hex() == c["after"]
    # ---- without the encodings: the same terms, the state not looked at
    assert emulate(N, ell, a, k, bl)[:3] == (tb, sc, offs)


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_term_lists_give_the_reference_points(native_lib, cases, which):
    """ell = 1, 2, 5, 8: every term list, evaluated by the oracle over the fixture's bases, is the proof's point."""
    c = cases[which]
    ell = c["ell"]
    dec = lambda h: O.g1_decompress(bytes.fromhex(h))
    bases = [dec(c["crs_G_t"]), dec(c["crs_G_u"]), dec(c["crs_H"])] + [dec(h) for h in c["vec_R"]] + [dec(h) for h in c["vec_S"]]
    tb, sc, offs, _, _ = emulate(native_lib, ell, [le(h) for h in c["vec_a"]], le(c["k"]), blinders(c))
    enc = encodings(c)
    for q in range(10):
        acc = None
        for t, s in zip(tb[offs[q]: offs[q + 1]], sc[offs[q]: offs[q + 1]]):
            acc = O.g1_add(acc, O.g1_mul(bases[t], s))
        assert O.g1_compress(acc) == enc[48 * q: 48 * q + 48], (ell, q)


def test_refusals(native_lib, cases):
    N = native_lib
    assert N.cg1_same_scalar_proof_bytes() == 576
    c = cases[2]
    ell, a, k, bl = c["ell"], [le(h) for h in c["vec_a"]], le(c["k"]), blinders(c)
    enc = encodings(c)
    start = start_state(N, c).raw

    def refused(want, ell_=ell, a_=a, k_=k, bl_=bl, enc_=enc):
        st = ctypes.create_string_buffer(start, 208)
        emulate(N, ell_, a_, k_, bl_, enc_, st, want=want)
        assert st.raw == start

    for bad in (R, R + 5, (1 << 256) - 1):                               # a scalar >= r is refused, never reduced
        refused(N.ERR_ENCODING, a_=a[:-1] + [bad])
        refused(N.ERR_ENCODING, k_=bad)
        for i in range(5):
            refused(N.ERR_ENCODING, bl_=bl[:i] + [bad] + bl[i + 1:])
    refused(N.ERR_ARG, ell_=0, a_=[])
    refused(N.ERR_ARG, ell_=N.SAME_SCALAR_MAX_ELL + 1, a_=[1] * (N.SAME_SCALAR_MAX_ELL + 1))
    refused(N.ERR_ENCODING, enc_=bytes([enc[0] & 0x7F]) + enc[1:])       # R without the compression flag
    refused(N.ERR_ENCODING, enc_=enc[:48 * 9] + b"\x9f" + b"\xff" * 47)  # B.T_2 with x >= p
    st = ctypes.create_string_buffer(start, 208)                          # and a good call still gives the fixture's alpha
    assert emulate(N, ell, a, k, bl, enc, st)[3] == le(c["alpha"]) and st.raw != start
    # ---- the C entry's refusals that need no GPU: they come before a context is looked at
    assert N.cg1_same_scalar_prove_device(None, None, ell, 1, None, None, None, None, None, 0, None, None, None) == N.ERR_HIP


def test_an_identity_encoding_is_absorbed_canonically(native_lib, cases):
    """An encoding with the infinity flag and stray bits is absorbed as C0 00 .. 00, as the reference re-serialises it (util.py:27-32)."""
    N, c = native_lib, cases[1]
    ell, a, k, bl = c["ell"], [le(h) for h in c["vec_a"]], le(c["k"]), blinders(c)
    enc = encodings(c)
    canon, stray = b"\xc0" + bytes(47) + enc[48:], b"\xe0" + bytes(46) + b"\x01" + enc[48:]
    out = []
    for e in (canon, stray):
        st = start_state(N, c)
        out.append((emulate(N, ell, a, k, bl, e, st)[3], st.raw))
    assert out[0] == out[1] and out[0][0] != le(c["alpha"])


def test_symbol_lists_agree(native_lib):
    src = open(os.path.join(ROOT, "include", "curdle_g1.h")).read()
    stripped = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cg1_[a-z0-9_]+)\s*\(", stripped))
    lib = ctypes.CDLL(native_lib.LIB_PATH)
    for name in SSCALAR:
        assert name in declared and hasattr(lib, name) and name in native_lib.EXPORTED_SYMBOLS and callable(getattr(native_lib, name)), name
    assert sorted(native_lib.EXPORTED_SYMBOLS) == sorted(declared)
    for macro, value in (("CG1_SAME_SCALAR_MAX_ELL", native_lib.SAME_SCALAR_MAX_ELL), ("CG1_SAME_SCALAR_MAX_PROVERS", native_lib.SAME_SCALAR_MAX_PROVERS)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), stripped), macro
    assert re.search(r"#define\s+CG1_SAME_SCALAR_NOT_G1\s+0x%x\b" % native_lib.SAME_SCALAR_NOT_G1, stripped)
    assert native_lib.SAME_SCALAR_NOT_G1 == 2 * native_lib.SAME_PERM_BAD_M                                  # the next free bit of the chain's status word
    # one launch: 10 MSMs per prover, ell + 1 terms at most, 3 + P 2 ell bases (the largest batch at the shuffle's ell = 124 fits)
    assert 10 * native_lib.SAME_SCALAR_MAX_PROVERS <= native_lib.LIGHT_MAX_MSMS and native_lib.SAME_SCALAR_MAX_ELL + 1 <= native_lib.LIGHT_MAX_TERMS
    assert 3 + native_lib.SAME_SCALAR_MAX_PROVERS * 2 * 124 <= native_lib.LIGHT_MAX_BASES and 3 + 2 * native_lib.SAME_SCALAR_MAX_ELL <= native_lib.LIGHT_MAX_BASES
