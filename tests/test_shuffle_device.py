"""The device prover of a whole shuffle proof, the parts that run without a GPU: the proof length, the formulas and term schedule
k_shuffle_begin runs (cg1_shuffle_begin_emulate is compiled from csrc/shuffle_rounds.h, the header the kernel includes) against Python
ints, and the reference's own CurdleProofsProof.new as recorded in tests/golden/shuffle_device_vectors.json cut at the offsets the entry
assembles a proof at and rebuilt from a chain of the three existing emulators with the CPU oracle's MSMs -- which pins the assembly order
and the identity A' = MSM(vec_G | vec_H[:2] | G_t | G_u, vec_x) without a GPU -- plus the symbol lists."""
import ctypes
import json
import os
import random
import re

import pytest

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = O.R
NB = 4
SHUFFLE = ["cg1_shuffle_prover_proof_bytes", "cg1_shuffle_prove_device", "cg1_shuffle_begin_emulate"]
ELLS = [4, 12, 28, 124]
# the same-scalar block's 48-byte slots in the transcript's order R, S, T.T_1, T.T_2, U.T_1, U.T_2, A.T_1, A.T_2, B.T_1, B.T_2
SLOTS = [4, 5, 0, 1, 2, 3, 6, 7, 8, 9]


@pytest.fixture(scope="module")
def cases():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "shuffle_device_vectors.json")))["cases"]


def s32(values):
    return b"".join(v.to_bytes(32, "little") for v in values)


def ints(raw, n):
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(n)]


def le(h):
    return int.from_bytes(bytes.fromhex(h), "little")


def draws_of(case):
    d = case["draws"]
    return {key: ([le(h) for h in v] if isinstance(v, list) else le(v)) for key, v in d.items()}


def begin_emulate(N, ell, a, perm, k, bl, abl, gi_a, gi_m, want=0):
    """-> (tb, sc, offs, vec_x, ss_tb, ss_sc, ss_offs) of cg1_shuffle_begin_emulate."""
    n, nt = ell + NB, 6 * ell + 8
    u32 = lambda v: (ctypes.c_uint32 * max(1, len(v)))(*v)
    tb, sc, offs, vx = (ctypes.c_uint32 * (2 * n))(), ctypes.create_string_buffer(64 * n), (ctypes.c_uint32 * 3)(), ctypes.create_string_buffer(32 * n)
    ss_tb, ss_sc, ss_offs = (ctypes.c_uint32 * nt)(), ctypes.create_string_buffer(32 * nt), (ctypes.c_uint32 * 11)()
    rc = N.cg1_shuffle_begin_emulate(ell, s32(a), u32(perm), s32([k]), s32(bl), s32(abl), u32(gi_a), u32(gi_m), tb, sc, offs, vx, ss_tb, ss_sc, ss_offs)
    assert rc == want, rc
    return list(tb), ints(sc.raw, 2 * n), list(offs), ints(vx.raw, n), list(ss_tb), ints(ss_sc.raw, nt), list(ss_offs)


def test_fixture_shape(cases):
    assert [c["ell"] for c in cases] == ELLS
    assert [c["permutation_kind"] for c in cases[:2]] == ["identity", "reversed"]
    for c in cases:
        ell, n = c["ell"], c["ell"] + NB
        assert ("vec_G" in c) == (ell <= 32) and len(c["vec_T"]) == len(c["vec_U"]) == len(c["permutation"]) == ell
        d = c["draws"]
        assert [len(d[key]) for key in ("vec_a_blinders", "vec_c_blinders", "ipa_r", "ipa_z_head", "vec_r")] == [2, NB, n, n - 2, n]


def test_proof_bytes(native_lib, cases):
    N = native_lib
    for ell in (0, 3, 5, N.SAME_MSM_MAX_N - NB + 1, 2 * N.SAME_MSM_MAX_N - NB, (1 << 64) - 2):
        assert N.cg1_shuffle_prover_proof_bytes(ell) == 0, ell
    assert N.cg1_shuffle_prover_proof_bytes(N.SAME_MSM_MAX_N - NB) != 0
    for c in cases:
        ell = c["ell"]
        assert N.cg1_shuffle_prover_proof_bytes(ell) == len(c["proof"]) // 2
        assert N.cg1_shuffle_prover_proof_bytes(ell) == 48 + 288 + N.cg1_same_perm_proof_bytes(ell, NB) + 288 + N.cg1_same_msm_proof_bytes(ell + NB)


@pytest.mark.parametrize("ell", [4, 12, 300])
def test_begin_against_python_ints(native_lib, ell):
    """The gather (with a permutation that is no bijection), the two scalar rows and their base rows, vec_x, and the same-scalar block's
    term lists, which are what cg1_same_scalar_emulate's begin produces.  At ell = 300 a lane of the kernel owns two elements."""
    N = native_lib
    rng = random.Random(700 + ell)
    n = ell + NB
    a, k, bl, abl = [rng.randrange(R) for _ in range(ell)], rng.randrange(R), [rng.randrange(R) for _ in range(5)], [rng.randrange(R) for _ in range(2)]
    perm = [rng.randrange(ell) for _ in range(ell)]
    perm[0] = perm[1] = ell - 1                                          # repeated entries: no bijection
    gi_a, gi_m = [1000 + j for j in range(n)], [1000 + j for j in range(ell + 2)] + [5000, 5001]
    tb, sc, offs, vx, ss_tb, ss_sc, ss_offs = begin_emulate(N, ell, a, perm, k, bl, abl, gi_a, gi_m)
    gathered = [a[m] for m in perm]
    assert offs == [0, n, 2 * n]
    assert vx == gathered + abl + bl[:2]
    assert sc[:n] == gathered + abl + [0, 0] and tb[:n] == gi_a          # the A row ends in two zeros
    assert sc[n:] == gathered + abl + bl[:2] and tb[n:] == gi_m          # the A' row ends in r_t, r_u, over G_t and G_u
    nt = 6 * ell + 8
    want_tb, want_sc, want_offs = (ctypes.c_uint32 * nt)(), ctypes.create_string_buffer(32 * nt), (ctypes.c_uint32 * 11)()
    assert N.cg1_same_scalar_emulate(ell, s32(a), s32([k]), s32(bl), None, None, want_tb, want_sc, want_offs, None, None) == N.OK
    assert (ss_tb, ss_sc, ss_offs) == (list(want_tb), ints(want_sc.raw, nt), list(want_offs))
    # ---- refusals: a permutation entry >= ell, a scalar >= r, a length outside 1 .. the limit
    begin_emulate(N, ell, a, perm[:-1] + [ell], k, bl, abl, gi_a, gi_m, want=N.ERR_ARG)
    begin_emulate(N, ell, a[:-1] + [R], perm, k, bl, abl, gi_a, gi_m, want=N.ERR_ENCODING)
    begin_emulate(N, ell, a, perm, k, bl, [abl[0], R + 1], gi_a, gi_m, want=N.ERR_ENCODING)
    assert N.cg1_shuffle_begin_emulate(0, *([None] * 14)) == N.ERR_ARG
    assert N.cg1_shuffle_prove_device(None, None, ell, 1, *([None] * 18), 0, None, None) == N.ERR_HIP      # before a context is looked at


def msm(points, scalars):
    acc = None
    for p, s in zip(points, scalars):
        acc = O.g1_add(acc, O.g1_mul(p, s))
    return acc


class Transcript:
    """The host transcript over a 208-byte state (cg1_merlin_*)."""

    def __init__(self, N, label):
        self.N, self.st = N, ctypes.create_string_buffer(N.MERLIN_STATE_BYTES)
        N.cg1_merlin_init(self.st, label, len(label))

    def append(self, label, msg):
        self.N.cg1_merlin_append(self.st, label, len(label), msg, len(msg))

    def append_list(self, label, items):
        self.N.cg1_merlin_append_list(self.st, label, len(label), b"".join(items), len(items[0]), len(items))

    def challenge(self, label):
        out = ctypes.create_string_buffer(32)
        self.N.cg1_merlin_challenge_scalar(self.st, label, len(label), out)
        return int.from_bytes(out.raw, "little")


@pytest.mark.parametrize("which", [0, 1])
def test_fixture_bytes_from_a_chain_of_the_three_emulators(native_lib, cases, which):
    """ell = 4 and 12: the recorded draws through cg1_shuffle_begin_emulate, cg1_same_perm_emulate, cg1_same_scalar_emulate and
    cg1_same_msm_round_emulate, every term list evaluated by the oracle, give the reference's bytes at the offsets the entry uses:
    A | cm_T cm_U R S | same_perm | cm_A cm_B z_k z_t z_u | same_msm.  Between the same-permutation head and the same-scalar block the
    transcript is replayed from the proof's own bytes (gprod_step1 .. the last ipa_gamma)."""
    N, c = native_lib, cases[which]
    ell, n = c["ell"], c["ell"] + NB
    lg = n.bit_length() - 1
    raw = bytes.fromhex(c["proof"])
    dec = lambda h: O.g1_decompress(bytes.fromhex(h))
    enc = O.g1_compress
    vec_G, vec_H, H, G_t, G_u = [dec(h) for h in c["vec_G"]], [dec(h) for h in c["vec_H"]], dec(c["H"]), dec(c["G_t"]), dec(c["G_u"])
    vR, vS, vT, vU = ([dec(h) for h in c[key]] for key in ("vec_R", "vec_S", "vec_T", "vec_U"))
    perm, k, mbl, d = list(c["permutation"]), le(c["k"]), [le(h) for h in c["vec_m_blinders"]], draws_of(c)
    bl = [d[key] for key in ("r_t", "r_u", "r_a", "r_b", "r_k")]
    pb_perm, pb_msm = N.cg1_same_perm_proof_bytes(ell, NB), N.cg1_same_msm_proof_bytes(n)
    o_perm, o_ss2, o_msm = 336, 336 + pb_perm, 336 + pb_perm + 288
    assert len(raw) == o_msm + pb_msm
    # ---- the head: curdleproofs_step1 [R + S + T + U], M, vec_a
    t = Transcript(N, b"curdleproofs")
    t.append_list(b"curdleproofs_step1", [bytes.fromhex(h) for key in ("vec_R", "vec_S", "vec_T", "vec_U") for h in c[key]])
    t.append(b"curdleproofs_step1", bytes.fromhex(c["M"]))
    a = [t.challenge(b"curdleproofs_vec_a") for _ in range(ell)]
    assert s32([a[0]]).hex() == c["vec_a_first"] and s32([a[-1]]).hex() == c["vec_a_last"]
    # ---- k_shuffle_begin's terms: table of the test = vec_G | vec_H | H | G_t | G_u
    table = vec_G + vec_H + [H, G_t, G_u]
    gi_a, gi_m = list(range(n)), list(range(ell + 2)) + [n + 1, n + 2]
    tb, sc, offs, vx, ss_tb, ss_sc, ss_offs = begin_emulate(N, ell, a, perm, k, bl, d["vec_a_blinders"], gi_a, gi_m)
    A = msm([table[i] for i in tb[:n]], sc[:n])
    A_prime = msm([table[i] for i in tb[n:]], sc[n:])
    assert enc(A) == raw[:48]
    light = [G_t, G_u, H] + vR + vS
    ss_pts = [msm([light[i] for i in ss_tb[ss_offs[q]: ss_offs[q + 1]]], ss_sc[ss_offs[q]: ss_offs[q + 1]]) for q in range(10)]
    ss_enc = [enc(p) for p in ss_pts]
    for q, slot in enumerate(SLOTS):                                     # cm_T | cm_U | R | S in front of the same-permutation proof, cm_A | cm_B behind it
        at = 48 + 48 * slot if slot < 6 else o_ss2 + 48 * (slot - 6)
        assert raw[at: at + 48] == ss_enc[q], q
    assert enc(O.g1_add(O.g1_add(A, ss_pts[2]), ss_pts[4])) == enc(A_prime)                # A' = A + cm_T.T_1 + cm_U.T_1 (curdleproofs.py:118)
    # ---- the same-permutation head and its first launch: A' = A, M' = M, B, C
    u32 = lambda v: (ctypes.c_uint32 * len(v))(*v)
    ab, b_out, gres = ctypes.create_string_buffer(64), ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32)
    ptb, psc, poffs, pst = (ctypes.c_uint32 * (4 * n))(), ctypes.create_string_buffer(128 * n), (ctypes.c_uint32 * 5)(), ctypes.c_uint32(0)
    assert N.cg1_same_perm_emulate(ell, NB, t.st, raw[:48], bytes.fromhex(c["M"]), s32(a), u32(perm), s32(d["vec_a_blinders"] + [0, 0]), s32(mbl),
                                   s32(d["vec_c_blinders"]), u32(gi_a), ab, b_out, gres, ptb, psc, poffs, ctypes.byref(pst)) == N.OK
    psc = ints(psc.raw, 4 * n)
    four = [msm([table[i] for i in list(ptb)[poffs[q]: poffs[q + 1]]], psc[poffs[q]: poffs[q + 1]]) for q in range(4)]
    B, C = four[2], four[3]
    assert [enc(p) for p in four] == [raw[:48], bytes.fromhex(c["M"]), raw[o_perm: o_perm + 48], raw[o_perm + 48: o_perm + 96]]
    # ---- the rest of the same-permutation transcript, from the proof's bytes (grand_prod.py:44-61, :64-95; ipa.py:100-105, :136-139)
    sp = raw[o_perm: o_ss2]                                              # B | C | r_p | B_c B_d | L_C R_C L_D R_D x lg | c d
    gprod_result, r_p = int.from_bytes(gres.raw, "little"), int.from_bytes(sp[96:128], "little")
    t.append(b"gprod_step1", sp[:48]); t.append(b"gprod_step1", gres.raw)
    g_alpha = t.challenge(b"gprod_alpha")
    t.append(b"gprod_step2", sp[48:96]); t.append(b"gprod_step2", sp[96:128])
    beta = t.challenge(b"gprod_beta")
    beta_inv = pow(beta, -1, R)
    G_prime = [O.g1_mul(G, pow(beta_inv, i + 1, R)) for i, G in enumerate(vec_G)]
    H_prime = [O.g1_mul(Hh, pow(beta_inv, ell + 1, R)) for Hh in vec_H]
    D = O.g1_add(O.g1_add(B, O.g1_neg(msm(G_prime, [pow(beta, i, R) for i in range(ell)]))), msm(H_prime, [g_alpha * pow(beta, ell + 1, R) % R] * NB))
    inner = (r_p * pow(beta, ell + 1, R) + gprod_result * pow(beta, ell, R) - 1) % R
    ipa = sp[128:]
    pt = lambda j: ipa[48 * j: 48 * j + 48]
    t.append_list(b"ipa_step1", [enc(C), enc(D)]); t.append(b"ipa_step1", s32([inner])); t.append_list(b"ipa_step1", [pt(0), pt(1)])
    t.challenge(b"ipa_alpha"); t.challenge(b"ipa_beta")
    for r in range(lg):                                                  # ipa_loop [L_C, L_D, R_C, R_D]
        t.append_list(b"ipa_loop", [pt(2 + r), pt(2 + 2 * lg + r), pt(2 + lg + r), pt(2 + 3 * lg + r)])
        t.challenge(b"ipa_gamma")
    # ---- the same-scalar block's transcript step and responses
    nt = 6 * ell + 8
    alpha, z = ctypes.create_string_buffer(32), ctypes.create_string_buffer(96)
    assert N.cg1_same_scalar_emulate(ell, s32(a), s32([k]), s32(bl), b"".join(ss_enc), t.st, (ctypes.c_uint32 * nt)(), ctypes.create_string_buffer(32 * nt),
                                     (ctypes.c_uint32 * 11)(), alpha, z) == N.OK
    assert z.raw == raw[o_ss2 + 192: o_ss2 + 288]
    # ---- the same-MSM argument over vec_G | vec_H[:2] | G_t | G_u and T | O O H O, U | O O O H, with vec_x as k_shuffle_begin left it
    G_m = [table[i] for i in gi_m]
    TU = vT + [None, None, H, None] + vU + [None, None, None, H]
    assert enc(msm(G_m, vx)) == enc(A_prime) and enc(msm(TU[:n], vx)) == ss_enc[3] and enc(msm(TU[n:], vx)) == ss_enc[5]      # Z_t = cm_T.T_2, Z_u = cm_U.T_2
    t.append_list(b"same_msm_step1", [enc(A_prime), ss_enc[3], ss_enc[5]])
    t.append_list(b"same_msm_step1", [enc(p) for p in TU])
    x, kk, r32, gi = ctypes.create_string_buffer(s32(vx), 32 * n), ctypes.create_string_buffer(s32([1] * n), 32 * n), s32(d["vec_r"]), u32([100 + j for j in range(n)])
    length = [n]

    def smsm(op, challenge=None):
        nm = 3 if op == 0 else 6
        mtb, msc, moffs = (ctypes.c_uint32 * (3 * n))(), ctypes.create_string_buffer(96 * n), (ctypes.c_uint32 * (nm + 1))()
        assert N.cg1_same_msm_round_emulate(op, n, length[0], x, kk, None if challenge is None else s32([challenge]), r32, gi, mtb, msc, moffs) == N.OK
        if op == 2:
            length[0] //= 2
        msc = ints(msc.raw, 3 * n)
        fixed_list = lambda q: q % 3 == 0
        return [enc(msm([G_m[i - 100] if fixed_list(q) else TU[i] for i in list(mtb)[moffs[q]: moffs[q + 1]]], msc[moffs[q]: moffs[q + 1]])) for q in range(nm)]

    sm = raw[o_msm:]
    mp = lambda j: sm[48 * j: 48 * j + 48]
    Bs = smsm(0)
    assert Bs == [mp(0), mp(1), mp(2)]
    t.append_list(b"same_msm_step1", Bs)
    smsm(1, t.challenge(b"same_msm_alpha"))
    for r in range(lg):                                                  # same_msm_loop [L_A, L_T, L_U, R_A, R_T, R_U]
        pts = [mp(3 + q * lg + r) for q in range(6)]
        t.append_list(b"same_msm_loop", pts)
        assert smsm(2, t.challenge(b"same_msm_gamma")) == pts, r
    assert x.raw[:32] == sm[-32:]                                        # x_final


def test_symbol_lists_agree(native_lib):
    src = open(os.path.join(ROOT, "include", "curdle_g1.h")).read()
    stripped = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cg1_[a-z0-9_]+)\s*\(", stripped))
    lib = ctypes.CDLL(native_lib.LIB_PATH)
    for name in SHUFFLE:
        assert name in declared and hasattr(lib, name) and name in native_lib.EXPORTED_SYMBOLS and callable(getattr(native_lib, name)), name
    assert sorted(native_lib.EXPORTED_SYMBOLS) == sorted(declared)
    # 64 provers at ell = 124: the T | U table, the R | S table and the ten MSMs per prover fit one call
    assert native_lib.SAME_MSM_MAX_PROVERS * 2 * 128 <= native_lib.LIGHT_MAX_BASES and 3 + native_lib.SAME_MSM_MAX_PROVERS * 2 * 124 <= native_lib.LIGHT_MAX_BASES
    assert native_lib.SAME_MSM_MAX_PROVERS <= native_lib.SAME_SCALAR_MAX_PROVERS and native_lib.SAME_MSM_MAX_N <= native_lib.IPA_MAX_N
