"""tests/prover_model.py, and through it the host emulations of the step kernels at vector lengths above their thread count.  No GPU.

1. The model over oracle points reproduces the reference's recorded proofs and final transcript states: every case of
   tests/golden/ipa_device_vectors.json and same_msm_device_vectors.json (n = 2, 8, 32, 128; both G' forms, both T | U shapes).
2. Over discrete logs it gives the bytes it gives over oracle points (n = 4, 16, 64): the cheap group is the same protocol.
3. cg1_ipa_round_emulate, cg1_same_msm_round_emulate and cg1_gprod_emulate -- compiled from the headers the kernels include -- at
   n0 = 1024 and 2048 with repeated table indices: the blinded and every folded vector, the final scalars, and every round's term lists
   summed in discrete logs against the points of the model, which folds its bases where the kernels keep coefficients.

Measured on a CPU-only machine: 6.4 s for the file.  The slowest: the two groups at n = 64, 1.4 s (oracle points fold 64 + 3 x 64 bases);
the recorded same-MSM proofs at n = 128, 0.9 s each; the recorded IPA proofs at n = 128, 0.6 s; every emulation test under 0.4 s."""
import ctypes
import hashlib
import json
import os
import random

import pytest

import prover_model as PM
from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = O.R


def le(h):
    return int.from_bytes(bytes.fromhex(h), "little")


def dec(h):
    return O.g1_decompress(bytes.fromhex(h))


def s32(values):
    return b"".join(v.to_bytes(32, "little") for v in values)


def ints(raw, n):
    return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(n)]


def golden(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))["cases"]


def start(case):
    return PM.transcript(case["label"].encode(), case["prefix_label"].encode(), bytes.fromhex(case["prefix"]))


# ---- 1. the recorded proofs
@pytest.mark.parametrize("which", range(6))
def test_ipa_model_reproduces_the_recorded_proofs(which):
    case = golden("ipa_device_vectors.json")[which]
    grp, n = PM.OraclePoints(), case["n"]
    G, Gp = [dec(h) for h in case["crs_G_vec"]], [dec(h) for h in case["crs_G_prime_vec"]]
    if case["form"] == "coeffs":                                         # G'[i] = beta^-(i+1) G[i]: built here, and it is what the reference recorded
        Gp = [grp.mul(G[i], pow(le(case["beta_inv"]), i + 1, R)) for i in range(n)]
        assert [grp.encode(p).hex() for p in Gp] == case["crs_G_prime_vec"]
    vec = lambda key: [le(h) for h in case[key]]
    got = PM.ipa_prove(grp, G, Gp, dec(case["crs_H"]), bytes.fromhex(case["C"]), bytes.fromhex(case["D"]), le(case["z"]), vec("vec_c"), vec("vec_d"),
                       vec("vec_r_c"), vec("vec_r_d"), start(case))
    want = bytes.fromhex(case["proof"])
    assert got.proof == want, (n, case["form"], PM.first_difference(got.names, got.proof, want))
    assert got.after.hex() == case["after"]
    assert (got.challenges["alpha"], got.challenges["beta"], got.challenges["gammas"]) == (le(case["alpha"]), le(case["beta"]), [le(h) for h in case["gammas"]])


@pytest.mark.parametrize("which", range(6))
def test_same_msm_model_reproduces_the_recorded_proofs(which):
    case = golden("same_msm_device_vectors.json")[which]
    G, T, U = ([dec(h) for h in case[k]] for k in ("crs_G_vec", "vec_T", "vec_U"))
    got = PM.same_msm_prove(PM.OraclePoints(), G, bytes.fromhex(case["A"]), bytes.fromhex(case["Z_t"]), bytes.fromhex(case["Z_u"]), T, U,
                            [le(h) for h in case["vec_x"]], [le(h) for h in case["vec_r"]], start(case))
    want = bytes.fromhex(case["proof"])
    assert got.proof == want, (case["n"], case["shape"], PM.first_difference(got.names, got.proof, want))
    assert got.after.hex() == case["after"]
    assert (got.challenges["alpha"], got.challenges["gammas"]) == (le(case["alpha"]), [le(h) for h in case["gammas"]])


def test_first_difference_names_the_slot():
    names = PM.ipa_slots(4)
    assert names == ["B_c", "B_d", "L_C[0]", "L_C[1]", "R_C[0]", "R_C[1]", "L_D[0]", "L_D[1]", "R_D[0]", "R_D[1]", "c_final", "d_final"]
    a = bytes(range(256)) * 3
    a = a[: 10 * 48 + 64]
    flip = lambda at: a[:at] + bytes([a[at] ^ 1]) + a[at + 1:]
    assert PM.first_difference(names, a, a) is None
    assert PM.first_difference(names, flip(47), a) == "B_c" and PM.first_difference(names, flip(48), a) == "B_d"
    assert PM.first_difference(names, flip(3 * 48 + 5), a) == "L_C[1]" and PM.first_difference(names, flip(9 * 48), a) == "R_D[1]"
    assert PM.first_difference(names, flip(10 * 48 + 31), a) == "c_final" and PM.first_difference(names, flip(10 * 48 + 32), a) == "d_final"
    assert PM.first_difference(names, a + b"x", a) == "length"
    assert PM.same_msm_slots(2) == ["B_a", "B_t", "B_u", "L_A[0]", "L_T[0]", "L_U[0]", "R_A[0]", "R_T[0]", "R_U[0]", "x_final"]


# ---- 2. the two groups
def dlog_inputs(rng, n, pool_size):
    """Bases g * G with repeating index patterns over a pool of `pool_size` logs, and random vectors."""
    pool = [rng.randrange(1, R) for _ in range(pool_size)]
    rs = lambda m: [rng.randrange(R) for _ in range(m)]
    return pool, rs


@pytest.mark.parametrize("n", [4, 16, 64])
def test_discrete_logs_give_the_bytes_of_oracle_points(n):
    rng = random.Random(9100 + n)
    pool, rs = dlog_inputs(rng, n, 2 * n + 1)
    pts = [O.g1_mul(O.G1_GEN, g) for g in pool]
    c, d, rc, rd, x, r = rs(n), rs(n), rs(n), rs(n), rs(n), rs(n)
    if n == 16:
        d[3] = c[5] = rd[0] = 0
    C48, D48 = O.g1_compress(pts[0]), PM.INF                              # only hashed
    res = [PM.ipa_prove(grp, B[:n], B[n: 2 * n], B[2 * n], C48, D48, 77, c, d, rc, rd, PM.transcript(b"two groups", b"n", bytes([n])))
           for grp, B in ((PM.OraclePoints(), pts), (PM.DiscreteLogs(), pool))]
    assert res[0].proof == res[1].proof, PM.first_difference(res[0].names, res[1].proof, res[0].proof)
    assert res[0].after == res[1].after and res[0].challenges == res[1].challenges
    assert len(set(res[0].parts.values())) == len(res[0].names)           # no two slots alike: the comparison can tell them apart
    T, U = [(5 * j + 2) % (2 * n + 1) for j in range(n)], [(3 * j + 1) % (n // 2 + 1) for j in range(n)]          # U repeats; the identity among T
    pool0, pts0 = pool + [0], pts + [None]
    T[1] = len(pool)
    res = [PM.same_msm_prove(grp, B[:n], C48, D48, PM.INF, [B[j] for j in T], [B[j] for j in U], x, r, PM.transcript(b"two groups", b"n", bytes([n])))
           for grp, B in ((PM.OraclePoints(), pts0), (PM.DiscreteLogs(), pool0))]
    assert res[0].proof == res[1].proof, PM.first_difference(res[0].names, res[1].proof, res[0].proof)
    assert res[0].after == res[1].after and res[0].challenges == res[1].challenges


# ---- 3. the emulations above the thread count
class NoEncodings(PM.DiscreteLogs):
    """Discrete logs whose encodings are a hash of the log: a transcript has something to absorb and no point is ever computed.  The
    proofs are not proofs; the challenges are as good as any, and the scalars and points (as logs) are what the tests here compare."""

    def encode(self, a):
        return hashlib.sha384((a % R).to_bytes(32, "little")).digest()


def dlog_sum(logs, tb, sc, lo, hi):
    assert all(t >> 31 == 0 for t in tb[lo:hi])
    return sum(logs[t] * s for t, s in zip(tb[lo:hi], sc[lo:hi])) % R


@pytest.mark.parametrize("n", [1024, 2048])
def test_ipa_emulation_at_lengths_above_the_thread_count(native_lib, n):
    """Explicit G' with coefficients on top, repeated indices (a pool of 131 logs), every round: blind, terms, fold."""
    N = native_lib
    assert n <= N.IPA_MAX_N
    rng = random.Random(9200 + n)
    pool, rs = dlog_inputs(rng, n, 131)
    gi, gpi, hi = [(7 * j + 3) % 130 for j in range(n)], [(11 * j + 5) % 130 for j in range(n)], 130
    coef, c, d, rc, rd = rs(n), rs(n), rs(n), rs(n), rs(n)
    grp = NoEncodings()
    m = PM.ipa_prove(grp, [pool[j] for j in gi], [pool[g] * k % R for g, k in zip(gpi, coef)], pool[hi], PM.INF, PM.INF, 5, c, d, rc, rd, PM.transcript(b"emulate"))
    cb, db = ctypes.create_string_buffer(s32(c), 32 * n), ctypes.create_string_buffer(s32(d), 32 * n)
    kg, kgp = ctypes.create_string_buffer(s32([1] * n), 32 * n), ctypes.create_string_buffer(s32(coef), 32 * n)
    GI, GPI = (ctypes.c_uint32 * n)(*gi), (ctypes.c_uint32 * n)(*gpi)
    kh = s32([m.challenges["beta"]])

    def call(op, ln, challenge):
        nt, nm = (2 * n, 2) if op == 0 else (2 * n + 2, 4)
        tb, sc, offs = (ctypes.c_uint32 * nt)(), ctypes.create_string_buffer(32 * nt), (ctypes.c_uint32 * (nm + 1))()
        assert N.cg1_ipa_round_emulate(op, n, ln, cb, db, kg, kgp, kh, None if challenge is None else s32([challenge]), s32(rc), s32(rd), GI, GPI, hi, tb, sc, offs) == 0
        return list(tb), ints(sc.raw, nt), list(offs)

    tb, sc, offs = call(0, n, None)
    assert offs == [0, n, 2 * n]
    assert [dlog_sum(pool, tb, sc, offs[q], offs[q + 1]) for q in range(2)] == [grp.msm([pool[j] for j in gi], rc), grp.msm([pool[g] * k % R for g, k in zip(gpi, coef)], rd)]
    call(1, n, m.challenges["alpha"])
    assert (ints(cb.raw, n), ints(db.raw, n)) == m.blinded
    ln, h = n, n // 2
    for k, gamma in enumerate(m.challenges["gammas"]):
        tb, sc, offs = call(2, ln, gamma)
        assert offs == [0, h + 1, 2 * h + 1, 3 * h + 2, 4 * h + 2] and tb[h] == hi and tb[3 * h + 1] == hi
        assert tuple(dlog_sum(pool, tb, sc, offs[q], offs[q + 1]) for q in range(4)) == m.rounds[k]["points"], (n, k)
        ln //= 2
        assert (ints(cb.raw, ln), ints(db.raw, ln)) == (m.rounds[k]["c"], m.rounds[k]["d"]), (n, k)
    assert ln == 1 and (ints(cb.raw, 1)[0], ints(db.raw, 1)[0]) == m.finals


@pytest.mark.parametrize("n", [1024, 2048])
def test_same_msm_emulation_at_lengths_above_the_thread_count(native_lib, n):
    N = native_lib
    rng = random.Random(9300 + n)
    pool, rs = dlog_inputs(rng, n, 140)
    gi = [(7 * j + 3) % 140 for j in range(n)]
    T, U, x, r = rs(n), rs(n), rs(n), rs(n)                                # the per-proof bases: 2 n logs, each its own
    xb, kb, GI = ctypes.create_string_buffer(s32(x), 32 * n), ctypes.create_string_buffer(s32([1] * n), 32 * n), (ctypes.c_uint32 * n)(*gi)

    def call(op, ln, challenge, want=0):
        nt, nm = 3 * n, (3 if op == 0 else 6)
        tb, sc, offs = (ctypes.c_uint32 * nt)(), ctypes.create_string_buffer(32 * nt), (ctypes.c_uint32 * (nm + 1))()
        assert N.cg1_same_msm_round_emulate(op, n, ln, xb, kb, None if challenge is None else s32([challenge]), s32(r), GI, tb, sc, offs) == want
        return list(tb), ints(sc.raw, nt), list(offs)

    if n > N.SAME_MSM_MAX_N:                                              # 2048 is past the argument's declared limit: refused, nothing written
        assert N.SAME_MSM_MAX_N == 1024
        call(0, n, None, want=N.ERR_ARG)
        call(1, n, 5, want=N.ERR_ARG)
        assert xb.raw == s32(x)
        return
    grp = NoEncodings()
    m = PM.same_msm_prove(grp, [pool[j] for j in gi], PM.INF, PM.INF, PM.INF, T, U, x, r, PM.transcript(b"emulate"), encoded_TU=[PM.INF] * (2 * n))
    TU = T + U
    value = lambda tb, sc, offs, q: dlog_sum(pool if q % 3 == 0 else TU, tb, sc, offs[q], offs[q + 1])
    tb, sc, offs = call(0, n, None)
    assert offs == [0, n, 2 * n, 3 * n]
    assert [value(tb, sc, offs, q) for q in range(3)] == [grp.msm(V, r) for V in ([pool[j] for j in gi], T, U)]
    call(1, n, m.challenges["alpha"])
    assert ints(xb.raw, n) == m.blinded
    ln, h = n, n // 2
    for k, gamma in enumerate(m.challenges["gammas"]):
        tb, sc, offs = call(2, ln, gamma)
        assert offs == [q * h for q in range(7)]
        assert tuple(value(tb, sc, offs, q) for q in range(6)) == m.rounds[k]["points"], (n, k)
        ln //= 2
        assert ints(xb.raw, ln) == m.rounds[k]["x"], (n, k)
    assert ln == 1 and ints(xb.raw, 1)[0] == m.finals[0]


@pytest.mark.parametrize("ell, nb", [(1020, 4), (1019, 5), (2044, 4), (1793, 255)])
def test_grand_product_emulation_at_lengths_above_the_thread_count(native_lib, ell, nb):
    """The grand-product argument's scalars from its equations -- c the prefix products, r_p, d in the powers of beta, the base change
    beta^-(i+1), <c, d>, the two completed blinders -- and its five term lists in discrete logs: B, C, D, B_c, B_d."""
    N = native_lib
    n = ell + nb
    rng = random.Random(9400 + ell)
    pool = [rng.randrange(1, R) for _ in range(137)]
    gi = [(7 * j + 3) % 137 for j in range(n)]
    rs = lambda m: [rng.randrange(1, R) for _ in range(m)]
    b, bbl, cbl, r, zh, alpha, beta = rs(ell), rs(nb), rs(nb), rs(n), rs(n - 2), rng.randrange(1, R), rng.randrange(1, R)
    c, pre = [], 1
    for v in b:
        c.append(pre)
        pre = pre * v % R
    c += cbl
    GI = (ctypes.c_uint32 * n)(*gi)
    state, two = ctypes.create_string_buffer(32 * 4 * n), ctypes.create_string_buffer(64)
    tb, sc, offs, st = (ctypes.c_uint32 * (5 * n))(), ctypes.create_string_buffer(32 * 5 * n), (ctypes.c_uint32 * 6)(), ctypes.c_uint32(0xffffffff)
    assert N.cg1_gprod_emulate(ell, nb, s32([pre]), s32(b + bbl), s32(cbl), s32(r), s32(zh), s32([alpha]), s32([beta]), GI, state, two, tb, sc, offs, ctypes.byref(st)) == 0
    assert st.value == 0
    raw = state.raw
    got = dict(c=ints(raw, n), d=ints(raw[32 * n:], n), kgp=ints(raw[64 * n:], n), z=ints(raw[96 * n:], n))
    binv = pow(beta, -1, R)
    rba = [(v + alpha) % R for v in bbl]
    r_p = PM.inner(rba, cbl)
    d = [(b[j] * pow(beta, j + 1, R) - pow(beta, j, R)) % R for j in range(ell)] + [pow(beta, ell + 1, R) * v % R for v in rba]
    kgp = [pow(binv, j + 1, R) for j in range(ell)] + [pow(binv, ell + 1, R)] * nb
    omega, delta = (PM.inner(r, d) + PM.inner(zh, c[: n - 2])) % R, PM.inner(r[: n - 2], zh)
    inv_c = pow(c[n - 2], -1, R)
    last_z = (r[n - 2] * inv_c * omega - delta) * pow((-r[n - 2] * inv_c * c[n - 1] + r[n - 1]) % R, -1, R) % R
    z = zh + [-inv_c * (last_z * c[n - 1] + omega) % R, last_z]
    assert (PM.inner(r, d) + PM.inner(z, c)) % R == 0 and PM.inner(r, z) == 0
    assert got == dict(c=c, d=d, kgp=kgp, z=z)
    assert ints(two.raw, 2) == [r_p, (r_p * pow(beta, ell + 1, R) + pre * pow(beta, ell, R) - 1) % R] and ints(two.raw, 2)[1] == PM.inner(c, d)
    tb, sc = list(tb), ints(sc.raw, 5 * n)
    assert list(offs) == [q * n for q in range(6)] and all(t < 137 for t in tb)
    G = [pool[j] for j in gi]
    Gp = [g * k % R for g, k in zip(G, kgp)]
    assert [dlog_sum(pool, tb, sc, q * n, (q + 1) * n) for q in range(5)] == [PM.inner(G, b + bbl), PM.inner(G, c), PM.inner(Gp, d), PM.inner(G, r), PM.inner(Gp, z)]
