"""The device provers at every halving depth and at vector lengths above the step kernels' 256 threads.  Needs an MI355X.

The recorded fixtures stop at n = 128 for the inner-product and same-MSM arguments (odd depths only) and at n = 512 for the arguments on
top of them.  Here the reference is tests/prover_model.py over discrete logs: every base is g * G for a known g, the model folds its
bases as integers, and a point is computed by the CPU oracle only where a proof emits it.  tests/test_prover_model.py pins that model to
the reference's recorded bytes.  The device entries must give the model's proof bytes and the model's `after` challenge; a mismatch
names the first differing proof slot.

One table of 140 bases serves the file (CG1_FIXED_MAX_BASES = 1024 is what forces repeated indices from n = 512 on in any case): up to
n = 64 the indices are distinct, from n = 256 they repeat -- gi[j] = (7 j + 3) mod 139 and the like.  Prover counts come from the
header's constants: CG1_IPA_MAX_PROVERS; min(CG1_SAME_MSM_MAX_PROVERS, CG1_LIGHT_MAX_BASES / 2n).

What each test is the first to reach:
  test_ipa_explicit                   even depths 2, 4, 6, 8 of k_ipa_step; from n = 1024 a second trip of its half-length loops (fold,
                                      round_term, the partial sums of the LDS tree), four at n = 2048; the chained MSM shapes 4 x 1025
                                      terms at slice 32 and 2 x 2048 terms (CG1_FIXED_MAX_TERMS)
  test_ipa_coefficient_form           the same loops with kGp loaded from the caller's coefficients, n = 512 and 2048 directly
  test_ipa_three_provers_at_1024      several workgroups whose state rows are 1024 elements apart
  test_ipa_most_provers               M = 1024 = CG1_FIXED_MAX_MSMS in one chained launch (256 provers x 4 MSMs)
  test_ipa_both_inversions_at_1024    ipa_inv over ten rounds
  test_same_msm_sizes                 even depths, and k_smsm_step's loops past one trip (n = 1024: two)
  test_same_msm_limit_shapes          P * 2n = CG1_LIGHT_MAX_BASES exactly, at (64, 128) -- the shape the README times -- and (8, 1024)
  test_same_msm_one_prover_too_many   the refusal on either side of that bound
  test_grand_product_scan_shapes,
  test_same_permutation_scan_shapes   scan_products with per = 4 and 8, a ragged last block of three elements and of one; k_gprod_step
                                      and k_same_perm_begin at n0 = 1024 and 2048
  test_whole_shuffle                  k_shuffle_begin and the chain behind it at ell = 60 and 252 (6 and 8 rounds), both entries; at
                                      ell = 1020 every part of the chain at its declared limit, over a CRS that has to repeat bases

Measured on an MI355X: 33 tests in 7 s of pytest time, 0.5 s of it the table and the pool (once).  Per test: the inner-product tests
0.03 - 0.09 s each (n = 2048: 0.09 s; 256 provers: 0.07 s), three provers at 1024 with their runs alone 0.19 s; same-MSM 0.03 s (n = 4) to
0.27 s (n = 1024), the limit shapes 0.32 s (64 x 128) and 0.72 s (8 x 1024, most of it the model's three transcripts), the refusals 0.07 and
0.21 s; grand product 0.02 - 0.05 s, same permutation 0.04 - 0.16 s; the whole shuffle 0.13 s (ell = 60), 0.11 s (252), 0.21 s (1020).

A build whose k_ipa_step keeps only the last trip of the <c_L, d_R> partial sum fails exactly the inner-product tests from n = 1024 on,
each naming L_C[0]; the grand-product and same-permutation tests cannot see it -- their reference ends in the same kernel -- which is
why the inner-product tests pin that kernel at the same n.
"""
import ctypes
import os
import random
import sys
import types

import pytest

import prover_model as PM
from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu
R = O.R
INF = PM.INF
POOL = 140                                                               # bases g * G in the table; index POOL of the kit's lists: the identity
NB = 4


def fr32(s):
    return bytes(s.to_le_bytes())


def comp(p):
    return bytes(p.to_compressed_bytes())


def s32(values):
    return b"".join(v.to_bytes(32, "little") for v in values)


def rot(v, k):
    return v[k % len(v):] + v[:k % len(v)]


class Kit:
    """POOL known multiples of G: as logs, as encodings, as product objects, and the FixedBaseTable over them."""

    def __init__(self):
        from curdleproofs_pie_amd import G1Point
        from curdleproofs_pie_amd.fixed_base import FixedBaseTable

        rng = random.Random(20250)
        self.logs = [rng.randrange(1, R) for _ in range(POOL)] + [0]
        self.enc = [O.g1_compress(O.g1_mul(O.G1_GEN, g)) for g in self.logs[:POOL]] + [INF]
        self.objs = [G1Point.from_compressed_bytes_unchecked(e) for e in self.enc]
        self.table = FixedBaseTable(self.objs[:POOL])
        self.group = PM.DiscreteLogs()
        for g, e in zip(self.logs, self.enc):
            self.group._enc[g] = e

    def transcript(self, label, prefix):
        from curdleproofs_pie_amd.merlin import CurdleproofsTranscript

        t = CurdleproofsTranscript(label)
        t.append(b"prefix", prefix)
        return t


@pytest.fixture(scope="module")
def kit(native_lib):
    k = Kit()
    yield k
    k.table.close()


def scalars(vals):
    from curdleproofs_pie_amd import Scalar
    return [Scalar(v) for v in vals]


def check(names, got, want, t, what):
    """The proof bytes, then the challenge drawn after them: the transcript's final state."""
    slot = PM.first_difference(names, got, want.proof)
    assert slot is None, "%s: the proof first differs from the model in %s" % (what, slot)
    assert fr32(t.get_and_append_challenge(b"after")) == want.after, "%s: the transcript after the proof differs from the model's" % (what,)


# ---------------------------------------------------------------------------------------------------- the inner-product argument
def ipa_bytes(res):
    B_c, B_d, LC, RC, LD, RD, c_fin, d_fin = res
    return b"".join(comp(p) for p in [B_c, B_d] + LC + RC + LD + RD) + fr32(c_fin) + fr32(d_fin)


class IpaInputs:
    """One length's indices and vectors.  form "explicit": G' at table indices of its own; "coeffs": G'[j] = coef[j] * G[j], the table
    indices of G' pointing back at G."""

    def __init__(self, kit, n, form):
        self.kit, self.n, self.form = kit, n, form
        rng = random.Random(31000 + n + (7 if form == "coeffs" else 0))
        rs = lambda: [rng.randrange(R) for _ in range(n)]
        if 2 * n + 1 <= POOL:
            self.gi, self.gpi, self.hi = list(range(n)), list(range(n, 2 * n)), 2 * n
        else:
            self.gi, self.gpi, self.hi = [(7 * j + 3) % (POOL - 1) for j in range(n)], [(11 * j + 5) % (POOL - 1) for j in range(n)], POOL - 1
        self.coef = None
        if form == "coeffs":
            self.gpi, self.coef = self.gi, rs()
        self.c, self.d, self.rc, self.rd = rs(), rs(), rs(), rs()
        self.label = b"ipa sizes %d %s" % (n, form.encode())

    def vectors(self, k):
        return rot(self.c, k), rot(self.d, 2 * k), rot(self.rc, 3 * k), rot(self.rd, k)

    def hashed(self, k):
        """C, D and z are only hashed: two encodings of the pool (the identity among them) and <c, d>."""
        c, d, _, _ = self.vectors(k)
        return self.kit.enc[k % POOL], self.kit.enc[POOL if k % 3 == 1 else (k + 9) % POOL], PM.inner(c, d)

    def prover(self, k=0):
        c, d, rc, rd = (scalars(v) for v in self.vectors(k))
        C, D, z = self.hashed(k)
        return (self.gi, self.gpi, self.hi, C, D, scalars([z])[0], c, d, rc, rd) + ((scalars(self.coef),) if self.coef else ())

    def model(self, k=0):
        logs = self.kit.logs
        Gp = [logs[j] for j in self.gpi] if self.coef is None else [logs[j] * q % R for j, q in zip(self.gpi, self.coef)]
        C, D, z = self.hashed(k)
        return PM.ipa_prove(self.kit.group, [logs[j] for j in self.gi], Gp, logs[self.hi], C, D, z, *self.vectors(k),
                            PM.transcript(self.label, b"prefix", b"prover %d" % k))

    def transcript(self, k=0):
        return self.kit.transcript(self.label, b"prover %d" % k)


def ipa_alone(kit, n, form):
    from curdleproofs_pie_amd.prover_kernels import ipa_prove_device_many

    inp = IpaInputs(kit, n, form)
    t = inp.transcript()
    (res,) = ipa_prove_device_many(kit.table, [inp.prover()], [t])
    check(PM.ipa_slots(n), ipa_bytes(res), inp.model(), t, "ipa n = %d, %s" % (n, form))


@pytest.mark.parametrize("n", [4, 16, 64, 256, 1024, 2048])
def test_ipa_explicit(kit, n):
    ipa_alone(kit, n, "explicit")


@pytest.mark.parametrize("n", [512, 2048])
def test_ipa_coefficient_form(kit, n):
    ipa_alone(kit, n, "coeffs")


def test_ipa_three_provers_at_1024(kit):
    """Rotated vectors, different prefixes: each prover gets the model's bytes, which are what it gets alone."""
    from curdleproofs_pie_amd.prover_kernels import ipa_prove_device_many

    n = 1024
    inp = IpaInputs(kit, n, "explicit")
    ts = [inp.transcript(k) for k in range(3)]
    got = ipa_prove_device_many(kit.table, [inp.prover(k) for k in range(3)], ts)
    states = [bytes(t.strobe._st.raw) for t in ts]
    for k in range(3):
        check(PM.ipa_slots(n), ipa_bytes(got[k]), inp.model(k), ts[k], "prover %d of 3 at n = 1024" % k)
        t1 = inp.transcript(k)
        (alone,) = ipa_prove_device_many(kit.table, [inp.prover(k)], [t1])
        assert ipa_bytes(alone) == ipa_bytes(got[k]) and bytes(t1.strobe._st.raw) == states[k], k


@pytest.mark.parametrize("n", [2, 4])
def test_ipa_most_provers(native_lib, kit, n):
    """CG1_IPA_MAX_PROVERS provers in one call: first, middle and last against the model, all of them distinct and the same in a second call."""
    from curdleproofs_pie_amd.prover_kernels import ipa_prove_device_many

    P = native_lib.IPA_MAX_PROVERS
    assert 4 * P == native_lib.FIXED_MAX_MSMS
    inp = IpaInputs(kit, n, "explicit")
    # rotations alone repeat after n provers: every prover also gets a vector entry of its own
    def prover(k):
        pr = list(inp.prover(k))
        pr[6] = scalars([(v + k * k) % R for v in rot(inp.c, k)])
        return tuple(pr)

    def model(k):
        logs = kit.logs
        C, D, z = inp.hashed(k)
        c, d, rc, rd = inp.vectors(k)
        return PM.ipa_prove(kit.group, [logs[j] for j in inp.gi], [logs[j] for j in inp.gpi], logs[inp.hi], C, D, z, [(v + k * k) % R for v in c], d, rc, rd,
                            PM.transcript(inp.label, b"prefix", b"prover %d" % k))

    provers = [prover(k) for k in range(P)]
    ts = [inp.transcript(k) for k in range(P)]
    got = [ipa_bytes(g) for g in ipa_prove_device_many(kit.table, provers, ts)]
    assert len(got) == P and len(set(got)) == P
    for k in (0, P // 2, P - 1):
        check(PM.ipa_slots(n), got[k], model(k), ts[k], "prover %d of %d at n = %d" % (k, P, n))
    ts2 = [inp.transcript(k) for k in range(P)]
    assert [ipa_bytes(g) for g in ipa_prove_device_many(kit.table, provers, ts2)] == got
    for k in (1, P // 2 + 1, P - 2):                                      # the states of provers not drawn from above
        assert bytes(ts2[k].strobe._st.raw) == bytes(ts[k].strobe._st.raw) != bytes(inp.transcript(k).strobe._st.raw)


def test_ipa_both_inversions_at_1024(native_lib, kit):
    from curdleproofs_pie_amd.prover_kernels import ipa_prove_device

    n = 1024
    inp = IpaInputs(kit, n, "coeffs")
    want = inp.model()
    ctx = kit.table._ctx
    try:
        for mode in (1, 0):
            ctx.set_param("ipa_inv", mode)
            t = inp.transcript()
            pr = inp.prover()
            check(PM.ipa_slots(n), ipa_bytes(ipa_prove_device(kit.table, *pr[:10], t, G_prime_coeffs=pr[10])), want, t, "ipa_inv = %d at n = 1024" % mode)
    finally:
        ctx.set_param("ipa_inv", 0)


# ---------------------------------------------------------------------------------------------------- the same-MSM argument
def smsm_bytes(res):
    B_a, B_t, B_u, LA, LT, LU, RA, RT, RU, x_fin = res
    return b"".join(comp(p) for p in [B_a, B_t, B_u] + LA + LT + LU + RA + RT + RU) + fr32(x_fin)


class SmsmInputs:
    """vec_T and vec_U are pool objects by index pattern (index POOL: the identity, which both vectors hold once)."""

    def __init__(self, kit, n):
        self.kit, self.n = kit, n
        rng = random.Random(32000 + n)
        self.gi = list(range(n)) if n <= POOL else [(7 * j + 3) % (POOL - 1) for j in range(n)]
        self.ti, self.ui = [(5 * j + 2) % POOL for j in range(n)], [(3 * j + 1) % (POOL - 3) for j in range(n)]
        self.ti[1] = self.ui[n - 1] = POOL
        self.x, self.r = [rng.randrange(R) for _ in range(n)], [rng.randrange(R) for _ in range(n)]
        self.label = b"same-msm sizes %d" % n

    def parts(self, k):
        return rot(self.ti, k), rot(self.ui, 2 * k)[::-1 if k % 2 else 1], rot(self.x, k), rot(self.r, 3 * k)

    def hashed(self, k):
        e = self.kit.enc
        return e[k % POOL], e[POOL if k % 2 else (k + 1) % POOL], e[(k + 2) % POOL]

    def prover(self, k=0):
        ti, ui, x, r = self.parts(k)
        o = self.kit.objs
        return (self.gi, *self.hashed(k), [o[j] for j in ti], [o[j] for j in ui], scalars(x), scalars(r))

    def model(self, k=0):
        ti, ui, x, r = self.parts(k)
        logs, e = self.kit.logs, self.kit.enc
        return PM.same_msm_prove(self.kit.group, [logs[j] for j in self.gi], *self.hashed(k), [logs[j] for j in ti], [logs[j] for j in ui], x, r,
                                 PM.transcript(self.label, b"prefix", b"prover %d" % k), encoded_TU=[e[j] for j in ti + ui])

    def transcript(self, k=0):
        return self.kit.transcript(self.label, b"prover %d" % k)


@pytest.mark.parametrize("n", [4, 16, 64, 256, 512, 1024])
def test_same_msm_sizes(kit, n):
    from curdleproofs_pie_amd.prover_kernels import same_msm_prove_device_many

    inp = SmsmInputs(kit, n)
    t = inp.transcript()
    (res,) = same_msm_prove_device_many(kit.table, [inp.prover()], [t])
    check(PM.same_msm_slots(n), smsm_bytes(res), inp.model(), t, "same-MSM n = %d" % n)


def smsm_bound(N, n):
    """The most provers of length n one call carries: both constants of the header."""
    return min(N.SAME_MSM_MAX_PROVERS, N.LIGHT_MAX_BASES // (2 * n))


@pytest.mark.parametrize("n", [128, 1024])
def test_same_msm_limit_shapes(native_lib, kit, n):
    """(64, 128) and (8, 1024): P * 2n = CG1_LIGHT_MAX_BASES exactly.  First, middle and last prover against the model; all distinct."""
    from curdleproofs_pie_amd.prover_kernels import same_msm_prove_device_many

    N = native_lib
    P = smsm_bound(N, n)
    assert (P, n) in ((64, 128), (8, 1024)) and P * 2 * n == N.LIGHT_MAX_BASES
    inp = SmsmInputs(kit, n)
    ts = [inp.transcript(k) for k in range(P)]
    got = [smsm_bytes(g) for g in same_msm_prove_device_many(kit.table, [inp.prover(k) for k in range(P)], ts)]
    assert len(got) == P and len(set(got)) == P
    for k in (0, P // 2, P - 1):
        check(PM.same_msm_slots(n), got[k], inp.model(k), ts[k], "prover %d of %d at n = %d" % (k, P, n))


@pytest.mark.parametrize("n", [128, 1024])
def test_same_msm_one_prover_too_many(native_lib, kit, n):
    """One prover more than the bound allows: CG1_ERR_ARG with the entry's documented text, and neither the proofs nor the states are
    written (the pattern of test_same_msm_device_gpu.test_refusals_leave_everything_untouched); the bound itself then runs."""
    from curdleproofs_pie_amd.py_arkworks_bls12381 import points_to_affine96

    N = native_lib
    P = smsm_bound(N, n) + 1
    inp = SmsmInputs(kit, n)
    pr = inp.prover()
    pb = N.cg1_same_msm_proof_bytes(n)
    start = bytes(inp.transcript().strobe._st.raw)[:208]
    assert len(start) == 208
    tu = bytes(points_to_affine96(list(pr[4]) + list(pr[5])))
    x, r = s32(inp.x), s32(inp.r)

    def call(count):
        gi = (ctypes.c_uint32 * (n * count))(*(inp.gi * count))
        st = ctypes.create_string_buffer(start * count, 208 * count)
        out = ctypes.create_string_buffer(b"\xaa" * (pb * count), pb * count)
        rc = N.cg1_same_msm_prove_device(kit.table._ctx.handle, kit.table._tab.handle, n, count, gi, b"".join(pr[1:4]) * count, tu * count, x * count, r * count, st, out, None)
        return rc, st.raw, out.raw

    rc, st, out = call(P)
    text = N.cg1_ctx_error(kit.table._ctx.handle).decode()
    assert rc == N.ERR_ARG and text == "cg1_same_msm_prove_device: more than %d provers, or more than %d bases T | U, in one call" % (N.SAME_MSM_MAX_PROVERS, N.LIGHT_MAX_BASES), text
    assert st == start * P and out == b"\xaa" * (pb * P)
    rc, st, out = call(P - 1)                                             # the bound itself: P - 1 copies of one prover, one proof P - 1 times
    assert rc == N.OK and out == out[:pb] * (P - 1) and st == st[:208] * (P - 1) and st[:208] != start
    assert PM.first_difference(PM.same_msm_slots(n), out[:pb], inp.model().proof) is None


# ---------------------------------------------------------------------------------------------------- grand product, same permutation
SCAN_SHAPES = [(1020, 4), (1019, 5), (257, 255), (2044, 4)]              # per = 4 | a last block of three | per = 2, a last block of one | per = 8


def scan_indices(ell, nb):
    return [(7 * j + 3) % (POOL - 5) for j in range(ell)], [POOL - 5 + (j % 4) for j in range(nb)], POOL - 1


@pytest.mark.parametrize("ell,nb", SCAN_SHAPES)
def test_grand_product_scan_shapes(kit, ell, nb):
    """The device chain against the host-driven path of test_grand_product_device_gpu (Python ints, table.msm_many, the host transcript,
    then ipa_prove_device -- which the tests above pin at the same n), and C against the prefix products as Python integers."""
    from curdleproofs_pie_amd.prover_kernels import grand_product_prove_device
    from test_grand_product_device_gpu import host_driven, state, to_bytes

    n = ell + nb
    assert (ell + 255) // 256 in (2, 4, 8) and n in (512, 1024, 2048)
    rng = random.Random(33000 + ell)
    rs = lambda m: [rng.randrange(1, R) for _ in range(m)]
    gi, hi, ui = scan_indices(ell, nb)
    b, bbl, cbl, r, zh = rs(ell), rs(nb), rs(nb), rs(n), rs(n - 2)
    c, pre = [], 1
    for v in b:
        c.append(pre)
        pre = pre * v % R
    logs = [kit.logs[j] for j in gi + hi]
    B = kit.group.encode(PM.inner(logs, b + bbl))
    args = (gi, hi, ui, B, scalars([pre])[0], scalars(b), scalars(bbl), scalars(cbl), scalars(r), scalars(zh))
    label = b"gprod sizes %d %d" % (ell, nb)
    t_dev, t_host = kit.transcript(label, b"dev"), kit.transcript(label, b"dev")
    got = grand_product_prove_device(kit.table, *args, t_dev)
    want = host_driven(kit.table, *args, t_host)
    assert to_bytes(got) == to_bytes(want), (ell, nb)
    assert state(t_dev) == state(t_host), (ell, nb)
    assert comp(got[0]) == kit.group.encode(PM.inner(logs, c + cbl)), "C is not the commitment to the prefix products"
    assert comp(got[0]) != INF and pre != 0


@pytest.mark.parametrize("ell,nb", SCAN_SHAPES)
def test_same_permutation_scan_shapes(kit, ell, nb):
    """The device chain against the host-driven path of test_same_permutation_device_gpu; B and C against the factors and their prefix
    products as Python integers, the two challenges from the transcript model."""
    from curdleproofs_pie_amd.prover_kernels import same_permutation_prove_device
    from test_same_permutation_device_gpu import host_driven, state, to_bytes

    n = ell + nb
    rng = random.Random(34000 + ell)
    rs = lambda m: [rng.randrange(1, R) for _ in range(m)]
    gi, hi, ui = scan_indices(ell, nb)
    perm = rng.sample(range(ell), ell)
    a, abl, mbl, cbl, r, zh = rs(ell), rs(nb), rs(nb), rs(nb), rs(n), rs(n - 2)
    logs = [kit.logs[j] for j in gi + hi]
    A = kit.group.encode(PM.inner(logs, [a[m] for m in perm] + abl))
    M = kit.group.encode(PM.inner(logs, perm + mbl))
    args = (gi, hi, ui, A, M, scalars(a), perm, scalars(abl), scalars(mbl), scalars(cbl), scalars(r), scalars(zh))
    label = b"same-perm sizes %d %d" % (ell, nb)
    t_dev, t_host = kit.transcript(label, b"dev"), kit.transcript(label, b"dev")
    got = same_permutation_prove_device(kit.table, *args, t_dev)
    want = host_driven(kit.table, *args, t_host)
    assert to_bytes(got) == to_bytes(want), (ell, nb)
    assert state(t_dev) == state(t_host), (ell, nb)
    # the factors b_j = a[perm[j]] + perm[j] alpha + beta, their product and prefix products, from the model's transcript
    t = PM.transcript(label, b"prefix", b"dev")
    for item in [A, M] + [v.to_bytes(32, "little") for v in a]:
        t.append_message(b"same_perm_step1", item)
    alpha = int.from_bytes(t.challenge_scalar(b"same_perm_alpha"), "little")
    beta = int.from_bytes(t.challenge_scalar(b"same_perm_beta"), "little")
    b = [(a[m] + m * alpha + beta) % R for m in perm]
    bbl = [(x + alpha * y) % R for x, y in zip(abl, mbl)]
    c, pre = [], 1
    for v in b:
        c.append(pre)
        pre = pre * v % R
    B_dev, (C_dev, _, _) = got
    assert comp(B_dev) == kit.group.encode(PM.inner(logs, b + bbl)), "B is not the commitment to the factors"
    assert comp(C_dev) == kit.group.encode(PM.inner(logs, c + cbl)), "C is not the commitment to the prefix products"


# ---------------------------------------------------------------------------------------------------- the whole shuffle
SEED = bytes(range(100, 132))


class ShuffleKit:
    """A CRS and trackers out of the pool: vec_G repeats 129 bases from ell = 252 on, vec_H | H | G_t | G_u are seven more."""

    def __init__(self, kit, ell):
        o = kit.objs
        self.ell, self.table = ell, kit.table
        g = [o[j % 129] for j in range(ell)]
        self.crs = types.SimpleNamespace(vec_G=g, vec_H=o[129:133], H=o[133], G_t=o[134], G_u=o[135])
        self.vR = [o[(5 * j + 1) % POOL] for j in range(ell)]
        self.vS = [o[(9 * j + 4) % POOL] for j in range(ell)]
        self.pre = [(comp(r), comp(s)) for r, s in zip(self.vR, self.vS)]


@pytest.mark.parametrize("ell", [60, 252, 1020])
def test_whole_shuffle(native_lib, kit, ell):
    """shuffle_prove_device and ShuffleBatchProver.generate_packed (a fixed seed) against the composed path of
    test_shuffle_device_gpu.test_edge_inputs_against_the_composed_path; the batch verifier accepts both outputs, and rejects the one item
    whose post tracker was replaced by its negation."""
    from curdleproofs_pie_amd import Scalar
    from curdleproofs_pie_amd.prover_kernels import shuffle_prove_device
    from curdleproofs_pie_amd.shuffle_prover import ShuffleBatchProver, shuffle_draws_from_seed
    from curdleproofs_pie_amd.shuffle_verifier import are_valid_whisk_shuffle_proofs
    from test_shuffle_device_gpu import commit, composed, crs_bytes

    k = ShuffleKit(kit, ell)
    S = Scalar.from_le_bytes
    items = []
    # ---- shuffle_prove_device with draws of the test's own
    rng = random.Random(35000 + ell)
    rs = lambda m: scalars([rng.randrange(1, R) for _ in range(m)])
    draws = (rs(2), rs(NB), rs(ell + NB), rs(ell + NB - 2), *rs(5), rs(ell + NB))
    perm, kk, mbl = rng.sample(range(ell), ell), rs(1)[0], rs(NB)
    vT, vU, M = commit(k.crs, k.table, k.vR, k.vS, perm, kk, mbl)
    pr = (k.crs, k.vR, k.vS, vT, vU, M, perm, kk, mbl, draws)
    got = shuffle_prove_device(k.table, *pr)
    assert len(got) == native_lib.cg1_shuffle_prover_proof_bytes(ell)
    assert got == composed(k.table, *pr), ell
    items.append((k.pre, [(comp(t), comp(u)) for t, u in zip(vT, vU)], comp(M) + got))
    # ---- generate_packed: shuffle 0 of SEED draws what shuffle_draws_from_seed gives
    prover = ShuffleBatchProver(k.crs, table=k.table)
    post, proofs, status = prover.generate_packed(b"".join(r + s for r, s in k.pre), seed=SEED)
    assert status == [0] and len(post) == 96 * ell and len(proofs) == native_lib.cg1_whisk_shuffle_proof_bytes(ell)
    perm, kb, mblb, db = shuffle_draws_from_seed(SEED, 0, ell)
    assert sorted(perm) == list(range(ell))
    draws = tuple([S(x) for x in d] if isinstance(d, list) else S(d) for d in db)
    kk, mbl = S(kb), [S(x) for x in mblb]
    vT, vU, M = commit(k.crs, k.table, k.vR, k.vS, perm, kk, mbl)
    assert post == b"".join(comp(t) + comp(u) for t, u in zip(vT, vU))
    assert proofs == comp(M) + composed(k.table, k.crs, k.vR, k.vS, vT, vU, M, perm, kk, mbl, draws), ell
    items.append((k.pre, [(post[96 * i: 96 * i + 48], post[96 * i + 48: 96 * i + 96]) for i in range(ell)], proofs))
    # ---- the verifier
    crs = crs_bytes(k.crs)
    assert are_valid_whisk_shuffle_proofs(crs, items) == [True, True]
    for which in (0, 1):
        pre, post_l, proof = items[which]
        r_g = bytearray(post_l[ell // 2][0])
        r_g[0] ^= 0x20                                                   # the other y of the same x: a valid encoding of the negated point
        assert O.g1_decompress(bytes(r_g)) == O.g1_neg(O.g1_decompress(post_l[ell // 2][0]))
        bad = (pre, post_l[:ell // 2] + [(bytes(r_g), post_l[ell // 2][1])] + post_l[ell // 2 + 1:], proof)
        edited = [bad if i == which else it for i, it in enumerate(items)]
        assert are_valid_whisk_shuffle_proofs(crs, edited) == [i != which for i in range(2)]
