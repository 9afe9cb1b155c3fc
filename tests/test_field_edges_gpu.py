"""The device's Fp, G1 and Fr arithmetic, operation by operation, against big integers at the limb and carry edges whole MSMs and whole
proofs over random-looking data never reach (cg1_probe_fp_ops, cg1_probe_g1_ops, cg1_probe_fr_ops: raw limbs in, raw limbs out).

Every comparison is integer equality or a limb bound the headers state; there is no tolerance.  Launch sizes are not multiples of 4 or
of 64, so the tail rows / tail lanes of the probe kernels run too."""
import random

import numpy as np
import pytest

import field_edge_cases as F
import rowlane_model as M
from oracle import bls12_381 as O

pytestmark = pytest.mark.gpu

P, NL, MASK = M.P, 14, (1 << 28) - 1
NN = (1 << 28) + 3                              # nearly normal: limbs 0..12 of every row product (fp_row.h)
RP = (1 << 392) % P                             # the Montgomery radix
RINV = pow(RP, -1, P)
MUL, SQR, MUL2, NORM, IS_ZERO, INV, TO_WORDS, TO_HOST_WORDS = range(8)
LANE, ROW = 0, 1
TOP_P, TOP_2P, TOP_4P = P >> 364, (2 * P) >> 364, (4 * P) >> 364
HOSTR = M._const("D_HOSTR")
assert M.value(HOSTR) == (1 << 384) % P and O.P == P


@pytest.fixture(scope="module")
def dev(native_lib):
    ctx = native_lib.Context(0)
    yield native_lib, ctx
    ctx.close()


def fp_ops(dev, form, op, tuples, kmax=0):
    N, ctx = dev
    n = len(tuples)
    assert 0 < n <= 4096 and n % 4 and n % 64, n
    arr = np.zeros((n, 4, NL), dtype=np.uint32)
    for i, t in enumerate(tuples):
        for j, v in enumerate(t):
            arr[i, j] = v
    out, fl = np.full((n, NL), 0xFFFFFFFF, dtype=np.uint32), np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    ctx.check(N.cg1_probe_fp_ops(ctx.handle, form, op, kmax, arr.ctypes.data, n, out.ctypes.data, fl.ctypes.data))
    return [[int(v) for v in r] for r in out], [int(f) for f in fl]


def odd_count(tuples, filler):
    """Pad so that the count is no multiple of 4 or 64: the probe kernels' tails run."""
    tuples = list(tuples)
    while len(tuples) % 64 != 61:
        tuples.append(filler(len(tuples)))
    return tuples


# ---------------------------------------------------------------------------------------------------------------- operand classes
def operand_classes():
    """Limb vectors by class.  Every value is < 4.1p, so any product of two of them is far below the value precondition of a Montgomery
    product (a b + c d < p 2^392 ~ 2 520 p^2); what differs is where the LIMBS sit against each operation's limb precondition."""
    rng = random.Random(0xE1)
    c = {}
    # canonical values, strictly normal limbs: inside every precondition
    c["canonical"] = [M.limbs_of(v) for v in (0, 1, 2, P - 1, P - 2, (P + 1) // 2, (P - 1) // 2, RP, RP * RP % P, 1 << 380)]
    # the N-form boundary (what fp_mul may return): limbs 0..12 all 2^28 - 1 with the top limb zero / the largest that keeps the value < 2p,
    # and p, p + 1, 2p - 1 themselves
    c["nform_edge"] = [[MASK] * 13 + [0], [MASK] * 13 + [TOP_2P - 1], M.limbs_of(P), M.limbs_of(P + 1), M.limbs_of(2 * P - 1)]
    # nearly normal (what row_mul may return; value < 2p): every limb at 2^28 + 3, every limb at 2^28, and the full ripple -- a carry out of limb
    # 0 into twelve limbs of all ones.  fp_mul's own limb precondition (products <= 2^60) admits them too, so both forms get them
    c["nearly_normal"] = [[NN] * 13 + [TOP_2P - 2], [1 << 28] * 13 + [TOP_2P - 2], [1 << 28] + [MASK] * 12 + [TOP_2P - 2]]
    # the largest operand of a call site: P, R (row_add), M (row_dbl), qx, sx -- limbs 3 * 2^28 - 1, value <= 4.1p -- and the padded multiples
    c["site_max"] = [[3 * (1 << 28) - 1] * 13 + [TOP_4P], list(M.KP[3]), list(M.KP[6]), list(M.KP[12])]
    c["rand_n"] = [[rng.randrange(1 << 28) for _ in range(13)] + [rng.randrange(TOP_2P)] for _ in range(300)]
    c["rand_nn"] = [[rng.randrange(NN + 1) for _ in range(13)] + [rng.randrange(TOP_2P - 1)] for _ in range(300)]
    c["rand_lazy"] = [[rng.randrange(3 << 28) for _ in range(13)] + [rng.randrange(TOP_4P)] for _ in range(300)]
    c["rand_29"] = [[rng.randrange(1 << 29) for _ in range(13)] + [rng.randrange(TOP_4P)] for _ in range(300)]      # a lazy negation kp - x
    for k, vs in c.items():
        assert all(M.value(v) < 13 * P if k == "site_max" else M.value(v) <= 4.1 * P for v in vs), k
    c["edge"] = c["canonical"] + c["nform_edge"] + c["nearly_normal"] + c["site_max"]
    return c


def sparse_results(rng, count):
    """Products whose VALUE has zero limbs: b = T R / a for a sparse T above a b / 2^392 (~ p / 2 520 at most), so the product is T itself
    and not T + p.  A zero digit under a non-zero carry is what makes the first carry pass of a row product leave a limb of exactly
    2^28 -- the case the second pass exists for, which random operands meet about once in 2^25 products."""
    out = []
    sparse = [1 << 380, 1 << 372, 3 << 370, 0x1A000 << 364, (1 << 380) + 1, (1 << 375) + (1 << 28), (77 << 368) + (1 << 140), 1 << 379]
    for i in range(count):
        a = rng.randrange(1, P)
        b = sparse[i % len(sparse)] * RP * pow(a, -1, P) % P
        out.append((M.limbs_of(a), M.limbs_of(b)))
    return out


def mq(*prods):
    return M.montgomery_quotient(*[(M.value(a), M.value(b)) for a, b in prods])


def check_products(dev, op, tuples, prods_of, model_of):
    """One launch per form; the value, the limb bounds, row against lane, row against the model."""
    lane, _ = fp_ops(dev, LANE, op, tuples)
    rows, _ = fp_ops(dev, ROW, op, tuples)
    for i, t in enumerate(tuples):
        want = mq(*prods_of(t))
        assert M.value(lane[i]) == want and max(lane[i][:13]) < 1 << 28, (op, i, t, lane[i])
        assert M.value(rows[i]) == want and max(rows[i][:13]) <= NN, (op, i, t, rows[i])
        assert M.limbs_of(M.value(rows[i])) == lane[i], (op, i)                 # fp_norm of the row result: the one-lane result
        assert model_of(t)[:NL] == rows[i], (op, i, t, rows[i])                  # ties the model's overflow findings to the real code
        assert want < 2 * P


def test_mul_both_forms(dev):
    c = operand_classes()
    rng = random.Random(0xE2)
    sp = sparse_results(rng, 64)
    assert sum(M.mul(M.row(a), M.row(b), passes=1) != M.mul(M.row(a), M.row(b)) for a, b in sp) >= 48      # one carry pass is not enough there
    tuples = [(a, b) for a in c["edge"] for b in c["edge"]] + sp
    for k in ("rand_n", "rand_nn", "rand_lazy"):
        tuples += list(zip(c[k], c[k][1:] + c[k][:1]))
    tuples += [(a, b) for a, b in zip(c["rand_lazy"], c["rand_nn"])]             # stage 3 of row_add: P PP
    tuples = odd_count(tuples, lambda i: (c["rand_n"][i % 300], c["rand_lazy"][(i * 7) % 300]))
    assert max(max(a) * max(b) for a, b in tuples) <= 9 << 56                   # the limb precondition, both forms (fp_row.h: 13 * 2^56, fp28.h: 2^60)
    check_products(dev, MUL, tuples, lambda t: [t], lambda t: M.mul(M.row(t[0]), M.row(t[1])))


def test_sqr_both_forms(dev):
    c = operand_classes()
    tuples = [(a,) for a in c["edge"] + c["rand_n"] + c["rand_nn"] + c["rand_lazy"]]
    tuples = odd_count(tuples, lambda i: (c["rand_29"][i % 300],))
    assert max(max(a) for a, in tuples) < 1 << 30                               # fp_sqr's limb precondition
    check_products(dev, SQR, tuples, lambda t: [(t[0], t[0])], lambda t: M.mul(M.row(t[0]), M.row(t[0])))


def test_mul2_both_forms(dev):
    c = operand_classes()
    E, small = c["edge"], c["canonical"] + c["nform_edge"] + c["nearly_normal"]
    tuples = [(E[i % len(E)], E[(i // len(E)) % len(E)], small[i % len(small)], small[(i * 5 + 1) % len(small)]) for i in range(len(E) ** 2)]
    # the call sites of row_add stage 4 / row_dbl stage 3 at their maxima: limbs 3 * 2^28 - 1 against 3 * 2^28 - 1, plus 2^28 + 3 against kp6
    big, nn = c["site_max"][0], c["nearly_normal"][0]
    tuples += [(big, big, nn, list(M.KP[6])), (big, big, nn, list(M.KP[3])), (big, big, list(M.KP[6]), nn)]
    for k in ("rand_n", "rand_nn"):
        v = c[k]
        tuples += [(v[i], v[(i + 1) % 300], v[(i + 2) % 300], v[(i + 3) % 300]) for i in range(300)]
    tuples += [(c["rand_lazy"][i], c["rand_lazy"][(i + 1) % 300], c["rand_nn"][i], c["rand_29"][i]) for i in range(300)]
    tuples += [(a, b, M.limbs_of(0), M.limbs_of(0)) for a, b in sparse_results(random.Random(0xE3), 32)]       # row 3 / row 1 of those stages
    tuples = odd_count(tuples, lambda i: (c["rand_n"][i % 300], c["rand_lazy"][(i * 7) % 300], c["rand_nn"][(i * 3) % 300], c["rand_29"][(i * 11) % 300]))
    lim = max(max(a) * max(b) + max(x) * max(d) for a, b, x, d in tuples)
    assert lim <= 13 << 56 and 14 * lim + (14 << 56) < 1 << 64                  # fp_row.h's limb precondition | fp_mul2's
    check_products(dev, MUL2, tuples, lambda t: [(t[0], t[1]), (t[2], t[3])], lambda t: M.mul2(*[M.row(v) for v in t]))


def test_norm_both_forms(dev):
    c = operand_classes()
    rng = random.Random(0xE4)
    # any limbs whose carries do not wrap: u32 limbs with 16 to spare, top limb with room for the carry of limb 12
    huge = [[rng.randrange((1 << 32) - 16) for _ in range(13)] + [rng.randrange(1 << 31)] for _ in range(200)]
    huge += [[(1 << 32) - 17] * 13 + [(1 << 31) - 1], [1 << 28] + [MASK] * 12 + [0]]
    tuples = odd_count([(a,) for a in c["edge"] + c["rand_lazy"] + c["rand_29"] + huge], lambda i: (c["rand_nn"][i % 300],))
    lane, _ = fp_ops(dev, LANE, NORM, tuples)
    rows, _ = fp_ops(dev, ROW, NORM, tuples)
    for i, (a,) in enumerate(tuples):
        assert lane[i] == M.limbs_of(M.value(a)), (i, a)                         # value unchanged, limbs 0..12 < 2^28
        assert M.value(rows[i]) == M.value(a) and max(rows[i][:13]) <= NN, (i, a, rows[i])
        assert rows[i] == M.norm_pass(M.norm_pass(M.row(a)))[:NL], (i, a)


def test_inv_both_forms(dev):
    c = operand_classes()
    # a^(p-2) of a multiple of p is 0, which no product brings to R^2: the class leaves out 0 and p, the only such values below 2p
    ins = [a for a in c["canonical"] + c["nform_edge"] + c["nearly_normal"] if M.value(a) % P] + c["rand_n"][:100] + c["rand_nn"][:100]
    tuples = odd_count([(a,) for a in ins], lambda i: (c["rand_n"][100 + i % 200],))
    assert max(max(a) for a, in tuples) < 1 << 30                               # fp_inv starts with fp_sqr(a)
    lane, _ = fp_ops(dev, LANE, INV, tuples)
    rows, _ = fp_ops(dev, ROW, INV, tuples)
    for i, (a,) in enumerate(tuples):
        assert M.value(a) * M.value(lane[i]) % P == RP * RP % P, (i, a)          # (x R) (x^-1 R) = R^2
        assert max(lane[i][:13]) < 1 << 28 and M.value(lane[i]) < 2 * P
        assert max(rows[i][:13]) <= NN and M.limbs_of(M.value(rows[i])) == lane[i], (i, a)


def words_of(limbs12):
    return sum(w << (32 * j) for j, w in enumerate(limbs12))


def test_to_words_and_to_host_words(dev):
    c = operand_classes()
    rng = random.Random(0xE5)
    zero_reps = [M.limbs_of(k * P) for k in (1, 2, 3)] + [list(M.KP[3]), M.limbs_of(0)]       # the Montgomery image of each is exactly p (or 0)
    # a = p + 256 d lies in [p, 2p) and a 2^384 / 2^392 = d (mod p) with d below a 2^384 / 2^392's floor: fp_to_host_words' product comes out as
    # p + d >= p -- the `ge` branch -- and d picks how far the borrow of the subtraction runs: not at all | one limb | two | all thirteen
    ds = [0, 1, (1 << 28) - P % (1 << 28), (1 << 56) - P % (1 << 56), (1 << 364) - P % (1 << 364)] + [rng.randrange(1 << 360) for _ in range(40)]
    ge = [M.limbs_of(P + 256 * d) for d in ds]
    ins = zero_reps + ge + c["canonical"] + c["nform_edge"] + c["rand_n"] + c["rand_lazy"]
    tuples = odd_count([(a,) for a in ins], lambda i: (c["rand_29"][i % 300],))
    assert all(M.value(a) < 1 << 392 for a, in tuples)
    tw = [mq((a, M.limbs_of(1))) for a, in tuples]
    th = [mq((a, HOSTR)) for a, in tuples]
    assert sum(t == P for t in tw) >= 4                                                            # the `t == p` branch of fp_to_words
    borrows = [sum(1 for x, y in zip(M.limbs_of(t)[:13], M.D_P[:13]) if x < y) for t in th if t >= P]
    assert len(borrows) >= 40 and min(borrows) == 0 and max(borrows) >= 12                         # `ge`, and the borrow chain short and long
    got, _ = fp_ops(dev, LANE, TO_WORDS, tuples)
    goth, _ = fp_ops(dev, LANE, TO_HOST_WORDS, tuples)
    for i, (a,) in enumerate(tuples):
        v = M.value(a)
        assert got[i][12:] == [0, 0] and words_of(got[i][:12]) == v * RINV % P, (i, a)
        assert goth[i][12:] == [0, 0] and words_of(goth[i][:12]) == v * RINV * (1 << 384) % P, (i, a)


def test_is_zero_mod_p(dev):
    """True for every representation k p with k < kmax -- the padded tables themselves, p's limbs, normalised multiples -- false from
    kmax on, and false for k p + j 2^28 and k p + 2^364, whose limb 0 passes the fast path so that the slow path has to answer."""
    reps = {0: [M.limbs_of(0)], 1: [list(M.D_P)], 3: [list(M.KP[3])], 6: [list(M.KP[6])], 12: [list(M.KP[12])]}
    for k in range(2, 16):
        reps.setdefault(k, []).append(M.limbs_of(k * P))
    ins = [(k, v, True) for k, vs in sorted(reps.items()) for v in vs]
    near = []
    for k, v, _ in ins:                                                           # limb 0 untouched: the fast path says "k", the slow path must answer
        for j in (1, 2, 3):
            near.append((k, v[:1] + [v[1] + j] + v[2:], False))
        near.append((k, v[:13] + [v[13] + 1], False))
    rng = random.Random(0xE6)
    rnd = [(None, [rng.randrange(1 << 28) for _ in range(13)] + [rng.randrange(TOP_4P)], False) for _ in range(100)]
    cases = ins + near + rnd
    assert len(cases) % 4 and len(cases) % 64
    # kmax is a literal at every call site of the product code, and the probe offers those literals only (so that it is compiled from
    # nothing else): 6 -- xyzz_add's, quad_add's, row_add's -- on both forms; 8, 10 and 14 -- xyzz_madd's and xyzz_mmadd's -- on one lane,
    # the only form that passes them.  k runs from 0 to 15, past every one of them.
    for kmax, forms in ((6, (LANE, ROW)), (8, (LANE,)), (10, (LANE,)), (14, (LANE,))):
        for form in forms:
            _, flags = fp_ops(dev, form, IS_ZERO, [(v,) for _, v, _ in cases], kmax)
            for (k, v, zero), f in zip(cases, flags):
                assert zero == (M.value(v) % P == 0)
                assert f == (1 if zero and k < kmax else 0), (kmax, form, k, v)


# ------------------------------------------------------------------------------------------------------------------------ the group
def mont(v):
    return v * RP % P


def xyzz_values(pt, z, lift=(0, 0, 0, 0)):
    """(X, Y, ZZ, ZZZ) of the affine point with Z = z != 1, Montgomery form, coordinate i lifted by lift[i] p (N-form: still < 2p)."""
    x, y = pt
    vals = (x * z * z, y * z * z * z, z * z, z * z * z)
    return [mont(v % P) + l * P for v, l in zip(vals, lift)]


IDENTITY = ([[0] * NL] * 4, 1)


def record(limbs4, inf=0):
    return ([list(l) for l in limbs4], inf)


def pack(recs, normal):
    arr = np.zeros((len(recs), 64), dtype=np.uint32)
    for i, (limbs4, inf) in enumerate(recs):
        for j, l in enumerate(limbs4):
            arr[i, NL * j: NL * j + NL] = M.limbs_of(M.value(l)) if normal else l
        arr[i, 4 * NL] = inf
    return arr


def affine_of(rec64, limb_max):
    if rec64[4 * NL]:
        return None
    X, Y, ZZ, ZZZ = ([int(v) for v in rec64[NL * j: NL * j + NL]] for j in range(4))
    assert max(max(l[:13]) for l in (X, Y, ZZ, ZZZ)) <= limb_max
    xv, yv, zz, zzz = (M.value(l) for l in (X, Y, ZZ, ZZZ))
    assert xv < 11 * P and yv < 5 * P and zz < 2 * P and zzz < 2 * P            # the invariant of a stored xyzz (g1_xyzz.h)
    assert pow(zz * RINV, 3, P) == pow(zzz * RINV, 2, P) and zz % P
    return (xv * pow(zz, -1, P) % P, yv * pow(zzz, -1, P) % P)


def adversarial_point(rng):
    """A curve point whose Montgomery X has limbs 0..12 drawn from {0, 2^28 - 1, 2^28, 2^28 + 3} (nearly normal: as given, only rows can
    take it; the other forms get the same value normalised) at a random Z: the top limb is stepped until x^3 + 4 is a square.  Y, ZZ and
    ZZZ are strictly normal here; denormal_point has them nearly normal."""
    low = [rng.choice((0, MASK, 1 << 28, NN)) for _ in range(13)]
    top, z = rng.randrange(TOP_P), rng.randrange(2, P)
    while True:
        X = low + [top]
        x = M.value(X) * RINV * pow(z * z, -1, P) % P
        y = O.fp_sqrt((x * x * x + 4) % P)
        if y is not None:
            _, Yv, ZZv, ZZZv = xyzz_values((x, y), z)
            return (x, y), record([X, M.limbs_of(Yv), M.limbs_of(ZZv), M.limbs_of(ZZZv)])
        top += 1


def cube_root(a):
    """A cube root of a mod p, or None.  p - 1 = 9 t with 3 not dividing t: a^(1/3 mod t) is a root up to a ninth root of unity."""
    a %= P
    if a == 0:
        return 0
    if pow(a, (P - 1) // 3, P) != 1:
        return None
    t = (P - 1) // 9
    g = next(g for g in range(2, 50) if pow(g, (P - 1) // 3, P) != 1)
    c, x = pow(g, t, P), pow(a, pow(3, -1, t), P)
    for _ in range(9):
        if pow(x, 3, P) == a:
            return x
        x = x * c % P
    raise AssertionError("no cube root of a cubic residue")


DENORMAL = {                                                                      # limbs 0..12 of a nearly-normal coordinate: the field tests' patterns
    "all 2^28+3": lambda rng: [NN] * 13,
    "all 2^28": lambda rng: [1 << 28] * 13,
    "ripple": lambda rng: [1 << 28] + [MASK] * 12,
    "random": lambda rng: [rng.randrange(NN + 1) for _ in range(13)],
    "corners": lambda rng: [rng.choice((0, MASK, 1 << 28, NN)) for _ in range(13)],
}


def denormal_point(rng, kind, pattern):
    """A curve point as an XYZZ record with TWO coordinates given as chosen nearly-normal limbs (a row record may hold such limbs in any
    coordinate; only rows take them as given, the other forms get the same values normalised).  kind = (X or Y, ZZ or ZZZ): the Z
    coordinate's top limb is stepped until it is the square / the cube of some z, then the point coordinate's until the other affine
    coordinate exists on the curve (a square root for y, a cube root for x)."""
    pc, zc = kind
    low, top = DENORMAL[pattern](rng), rng.randrange(TOP_P)
    while True:
        Zl = low + [top]
        v = M.value(Zl) * RINV % P
        z = O.fp_sqrt(v) if zc == "ZZ" else cube_root(v)
        if z is not None and z > 1:
            break
        top += 1
    low, top = DENORMAL[pattern](rng), rng.randrange(TOP_P)
    while True:
        Pl = low + [top]
        v = M.value(Pl) * RINV % P
        if pc == "X":
            x = v * pow(z * z, -1, P) % P
            y = O.fp_sqrt((x * x * x + 4) % P)
        else:
            y = v * pow(z, -3, P) % P
            x = cube_root(y * y - 4)
        if x is not None and y is not None:
            break
        top += 1
    assert O.g1_is_on_curve((x, y))
    vals = xyzz_values((x, y), z)
    limbs = [M.limbs_of(v) for v in vals]
    for name, l in ((pc, Pl), (zc, Zl)):
        j = ("X", "Y", "ZZ", "ZZZ").index(name)
        assert M.value(l) % P == vals[j] and M.value(l) < 2 * P and max(l[:13]) <= NN
        limbs[j] = l
    return (x, y), record(limbs)


def same_x_pair(pt, rng):
    """Two representations a, b of pt (different Z) built so that U1 = X1 ZZ2 comes out of its Montgomery product as the canonical u
    and U2 = X2 ZZ1 as u + p: u sits just above p^2 / 2^392, above every product of two canonical operands and below the product of the two
    operands lifted by p.  Then U2 + (3p - U1) = 4p, and 2p with the operands swapped; ordinary pairs give 3p."""
    x, y = pt
    z1 = rng.randrange(2, P)
    u = (P * P >> 392) + 1
    while True:
        z2 = O.fp_sqrt(u * pow(x * z1 * z1 * RP, -1, P) % P)
        if z2 is not None and z2 not in (z1, P - z1):
            break
        u += 1
    a = xyzz_values(pt, z1, (0, 0, 1, 0))                                         # ZZ1 lifted
    b = xyzz_values(pt, z2, (1, 0, 0, 0))                                         # X2 lifted
    return a, b


def p_multiple(a_vals, b_vals):
    """Which multiple of p the code hands to is_zero_mod_p for a pair with equal x: U2 + (kp3 - U1), from the exact Montgomery quotients."""
    u1 = M.montgomery_quotient((a_vals[0], b_vals[2]))
    u2 = M.montgomery_quotient((b_vals[0], a_vals[2]))
    d = u2 + 3 * P - u1
    assert d % P == 0
    return d // P


def g1_cases():
    rng = random.Random(0xE7)
    pts = [O.g1_mul(O.G1_GEN, rng.randrange(1, O.R)) for _ in range(16)]
    rec = lambda vals: record([M.limbs_of(v) for v in vals])
    lifts = lambda: tuple(rng.randrange(2) for _ in range(4))
    cases, multiples = [], []                                                     # (a, b, expected a + b, expected 2 a)
    for i in range(96):                                                           # ordinary sums: canonical and value + p coordinates, Z != 1
        pa, pb = pts[i % 16], pts[(5 * i + 3) % 16 if (5 * i + 3) % 16 != i % 16 else (i + 1) % 16]
        lift_a, lift_b = ((0,) * 4, (0,) * 4) if i < 8 else (lifts(), lifts())
        cases.append((rec(xyzz_values(pa, rng.randrange(2, P), lift_a)), rec(xyzz_values(pb, rng.randrange(2, P), lift_b)), pa, pb))
    adv = [adversarial_point(rng) for _ in range(24)]
    for i, (pa, ra) in enumerate(adv):                                            # adversarial limbs as either operand, and on both sides
        pb = pts[i % 16]
        rb = rec(xyzz_values(pb, rng.randrange(2, P), lifts()))
        cases.append((ra, rb, pa, pb))
        cases.append((rb, ra, pb, pa))
        cases.append((ra, adv[(i + 1) % 24][1], pa, adv[(i + 1) % 24][0]))
    # nearly-normal Y, ZZ and ZZZ (and X again), two coordinates per record, every limb pattern: as either operand, on both sides, against
    # another representation of the same point and of its negative -- and, as every first operand, through the doubling
    den = [denormal_point(rng, kind, pat) for kind in (("Y", "ZZ"), ("Y", "ZZZ"), ("X", "ZZ"), ("X", "ZZZ")) for pat in DENORMAL]
    for i, (pa, ra) in enumerate(den):
        pb = pts[i % 16]
        rb = rec(xyzz_values(pb, rng.randrange(2, P), lifts()))
        pc, rc = den[(7 * i + 3) % len(den)]
        cases += [(ra, rb, pa, pb), (rb, ra, pb, pa), (ra, rc, pa, pc)]
        av = [M.value(l) for l in ra[0]]
        for neg in (False, True):
            bv = xyzz_values(pa, rng.randrange(2, P), lifts())
            if neg:
                bv = [bv[0], (-bv[1]) % P + (P if i % 2 else 0), bv[2], bv[3]]
            pn = O.g1_neg(pa) if neg else pa
            cases += [(ra, rec(bv), pa, pn), (rec(bv), ra, pn, pa)]
            multiples += [p_multiple(av, bv), p_multiple(bv, av)]
    for i in range(12):                                                           # P + P and P + (-P) from DIFFERENT representations of P
        pt = pts[i] if i % 3 else adv[i][0]
        for neg in (False, True):
            if i < 8:
                av, bv = same_x_pair(pt, rng)
            else:
                av, bv = xyzz_values(pt, rng.randrange(2, P), lifts()), xyzz_values(pt, rng.randrange(2, P), lifts())
            if neg:
                bv = [bv[0], (-bv[1]) % P + (P if i % 2 else 0), bv[2], bv[3]]   # -P: (X, -Y)
            pb = O.g1_neg(pt) if neg else pt
            for x, y, px, py in ((av, bv, pt, pb), (bv, av, pb, pt)):
                cases.append((rec(x), rec(y), px, py))
                multiples.append(p_multiple(x, y))
    ra = rec(xyzz_values(pts[0], rng.randrange(2, P), lifts()))
    cases += [(IDENTITY, ra, None, pts[0]), (ra, IDENTITY, pts[0], None), (IDENTITY, IDENTITY, None, None), (adv[0][1], IDENTITY, adv[0][0], None)]
    # P + P / P - P reach is_zero_mod_p(P, 6) with 2p, 3p and 4p: a kmax that is too small, or a slow path that compares with the wrong k p, shows
    assert set(multiples) == {2, 3, 4}, sorted(set(multiples))
    while len(cases) % 64 != 61:
        cases.append(cases[len(cases) % 96])
    return cases


@pytest.fixture(scope="module")
def g1_expected():
    cases = g1_cases()
    return cases, [O.g1_add(pa, pb) for _, _, pa, pb in cases], [O.g1_add(pa, pa) for _, _, pa, _ in cases]


@pytest.mark.parametrize("form", [0, 1, 2])
def test_group_operations_three_forms(dev, g1_expected, form):
    N, ctx = dev
    cases, want_add, want_dbl = g1_expected
    n = len(cases)
    assert n <= 4096 and n % 4 and n % 16 and n % 64
    normal = form != 2                                                            # only rows take nearly-normal limbs as they are
    arr = np.zeros((n, 2, 64), dtype=np.uint32)
    arr[:, 0] = pack([c[0] for c in cases], normal)
    arr[:, 1] = pack([c[1] for c in cases], normal)
    limb_max = NN if form == 2 else MASK
    for op, want in ((0, want_add), (1, want_dbl)):
        out = np.full((n, 64), 0xFFFFFFFF, dtype=np.uint32)
        ctx.check(N.cg1_probe_g1_ops(ctx.handle, form, op, arr.ctypes.data, n, out.ctypes.data))
        for i in range(n):
            assert int(out[i, 4 * NL]) in (0, 1)
            assert affine_of(out[i], limb_max) == want[i], (form, op, i)


# ------------------------------------------------------------------------------------------------------------------------------ Fr
def test_device_fr_against_ints_and_the_host_bytes(dev):
    N, ctx = dev
    device = lambda op, raw, n, out: N.cg1_probe_fr_ops(ctx.handle, op, raw, n, out)
    cases = F.fr_cases()
    assert sorted(cases) == list(range(10))
    ks = F.inv_binary_step_counts()
    assert {255, 256, 257} <= set(ks) and max(ks) >= 500 and any(333 <= k <= 395 for k in ks)
    for op, (ins, want) in cases.items():
        ins, want = list(ins), list(want)
        while len(ins) % 64 == 0 or len(ins) % 4 == 0:
            j = len(ins) % 7
            ins.append(ins[j]); want.append(want[j])
        raw = F.items(ins)
        got = F.run(device, op, raw)
        assert got == F.run(N.cg1_fr_ops_host, op, raw), op                        # byte for byte (F.run checks the padding bytes too)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (op, i, [hex(v) for v in ins[i]], hex(g[0]), hex(w[0]))
    r = F.R_MOD
    inv = cases[F.OP_INV][0]
    got_f = F.run(device, F.OP_INV, F.items(inv[:61]))
    got_b = F.run(device, F.OP_INV_BINARY, F.items(inv[:61]))
    assert got_f == got_b and got_f[0] == (0, 1)                                   # 0 -> 0, and the two inversions agree
    for (a, _), (g, _) in zip(inv[1:61], got_f[1:]):
        assert g == pow(a, -1, r) * F.R2 % r
