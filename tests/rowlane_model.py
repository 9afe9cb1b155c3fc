"""A bit-exact model of csrc/fp_row.h's field arithmetic -- one limb per lane over the 16 lanes of a DPP row -- in plain ints.

Every place where the C++ would silently wrap asserts here instead: a 64-bit accumulator, the `(uint32_t)(acc >> 28)` that keeps a column's
carry, every u32 limb sum, every limb-wise `kp - x` of a lazy subtraction.  The tests run it where fp_row.h's own callers run the real code
(tests/test_field_edges.py) and hold the device's limbs against its limbs (tests/test_field_edges_gpu.py).  The constants are read from
csrc/bls_consts.h, the file the device code is compiled from."""
import os
import re

NL, LANES, MASK = 14, 16, (1 << 28) - 1
_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "curdleproofs_pie_amd", "csrc", "bls_consts.h")


with open(_HDR) as _f:
    _TEXT = _f.read()


def _const(name):
    m = re.search(r"\b%s(\[\d+\])? = \{?([^;}]*)\}?;" % name, _TEXT)
    vals = [int(v.rstrip("ul"), 16) for v in re.findall(r"0x[0-9a-fA-F]+u?l*", m.group(2))]
    return vals if m.group(1) else vals[0]


D_P, D_PINV, D_R1, D_R2 = _const("D_P"), _const("D_PINV"), _const("D_R1"), _const("D_R2")
KP = {3: _const("D_KP3"), 6: _const("D_KP6"), 12: _const("D_KP12")}
U32, U64 = 1 << 32, 1 << 64


def value(limbs):
    return sum(int(v) << (28 * i) for i, v in enumerate(limbs))


def limbs_of(v):
    """The strictly normal limbs of v < 2^396 (limb 13 takes what is left)."""
    return [(v >> (28 * i)) & MASK for i in range(NL - 1)] + [v >> (28 * (NL - 1))]


P = value(D_P)
assert (P * D_PINV + 1) % (1 << 28) == 0 and all(value(KP[k]) == k * P for k in KP)


def row(limbs):
    """row_load14: lanes 14 and 15 hold zero."""
    assert len(limbs) == NL and all(0 <= v < U32 for v in limbs)
    return [int(v) for v in limbs] + [0] * (LANES - NL)


def u32(v):
    assert 0 <= v < U32, "a u32 sum wraps: %#x" % v
    return v


def norm_pass(t):
    """row_norm_pass: lane j keeps its low 28 bits (lane 13: everything) and takes the carry of lane j - 1 (row_shr:1, lane 0 <- 0)."""
    keep = [t[j] if j == 13 else t[j] & MASK for j in range(LANES)]
    c = [0 if j == 13 else t[j] >> 28 for j in range(LANES)]
    return [u32(keep[j] + (c[j - 1] if j else 0)) for j in range(LANES)]


def _step(t, i, pairs):
    """CG1_ROW_STEP / CG1_ROW_STEP2 number i: pairs = ((a, b),) or ((a, b), (c, d))."""
    acc = list(t)
    for a, b in pairs:
        acc = [a[j] * b[i] + acc[j] for j in range(LANES)]
        assert max(acc) < U64, "a 64-bit accumulator wraps"
    m = (((acc[0] & (U32 - 1)) * D_PINV) & (U32 - 1)) & MASK                      # lane 0's, broadcast
    acc = [m * (D_P[j] if j < NL else 0) + acc[j] for j in range(LANES)]
    assert max(acc) < U64, "a 64-bit accumulator wraps"
    assert max(a >> 28 for a in acc) < U32, "acc >> 28 does not fit the u32 it is kept in"
    low = [a & MASK for a in acc]
    return [u32((low[j + 1] if j + 1 < LANES else 0) + (acc[j] >> 28)) for j in range(LANES)], max(acc)      # row_shl:1, lane 15 <- 0


def mul2(a, b, c=None, d=None, passes=2, stats=None):
    """row_mul(a, b) / row_mul2(a, b, c, d) over rows of 16 lanes; `passes` carry passes at the end (the code: two)."""
    pairs = ((a, b),) if c is None else ((a, b), (c, d))
    t = [0] * LANES
    for i in range(NL):
        t, top = _step(t, i, pairs)
        if stats is not None:
            stats["acc"] = max(stats.get("acc", 0), top)
    for _ in range(passes):
        t = norm_pass(t)
    return t


def mul(a, b, **kw):
    return mul2(a, b, **kw)


def montgomery_quotient(*products):
    """(sum a b + q p) >> 392 with q = -(sum a b) p^-1 mod 2^392: the one value a Montgomery product of these operands may return."""
    s = sum(x * y for x, y in products)
    q = (-s * pow(P, -1, 1 << 392)) % (1 << 392)
    assert (s + q * P) % (1 << 392) == 0
    return (s + q * P) >> 392


def add(x, y):
    return [u32(x[j] + y[j]) for j in range(LANES)]


def neg(k, x):
    """kp - x limb by limb (fp_neg<k> on rows); lanes 14, 15: 0 - 0."""
    assert all(x[j] <= (KP[k][j] if j < NL else 0) for j in range(LANES)), "kp - x is negative in a limb"
    return [(KP[k][j] if j < NL else 0) - x[j] for j in range(LANES)]


def row_add(a, b, stats=None):
    """row_add's common path over rows X, Y, ZZ, ZZZ of a and of b; returns (X3, Y3, ZZ3, ZZZ3) and leaves its lazy values in `stats`."""
    (X1, Y1, ZZ1, ZZZ1), (X2, Y2, ZZ2, ZZZ2) = a, b
    U1, U2, S1, S2 = mul(X1, ZZ2), mul(X2, ZZ1), mul(Y1, ZZZ2), mul(Y2, ZZZ1)
    Pd, R = add(U2, neg(3, U1)), add(S2, neg(3, S1))
    PP, RR, ZZ12, ZZZ12 = mul(Pd, Pd, stats=stats), mul(R, R, stats=stats), mul(ZZ1, ZZ2), mul(ZZZ1, ZZZ2)
    PPP, Q, ZZ3 = mul(Pd, PP), mul(U1, PP), mul(ZZ12, PP)
    X3 = norm_pass(norm_pass(add(add(RR, neg(3, PPP)), [u32(2 * v) for v in neg(3, Q)])))
    qx, ns1 = add(Q, neg(12, X3)), neg(3, S1)
    Y3, ZZZ3 = mul2(R, qx, PPP, ns1, stats=stats), mul2(ZZZ12, PPP, [0] * LANES, [0] * LANES)
    if stats is not None:
        stats.update(P=Pd, R=R, qx=qx, ns1=ns1, X3=X3)
    return X3, Y3, ZZ3, ZZZ3


def row_dbl(a, stats=None):
    """row_dbl over rows X, Y, ZZ, ZZZ."""
    X, Y, ZZ, ZZZ = a
    U = add(Y, Y)
    V, XX = mul(U, U, stats=stats), mul(X, X)
    M = add(add(XX, XX), XX)
    W, S, MM, ZZ3 = mul(U, V), mul(X, V), mul(M, M, stats=stats), mul(V, ZZ)
    X3 = norm_pass(norm_pass(add(MM, [u32(2 * v) for v in neg(3, S)])))
    sx, ny = add(S, neg(12, X3)), neg(6, Y)
    Y3, ZZZ3 = mul2(M, sx, W, ny, stats=stats), mul2(W, ZZZ, [0] * LANES, [0] * LANES)
    if stats is not None:
        stats.update(M=M, sx=sx, ny=ny, X3=X3, U=U)
    return X3, Y3, ZZ3, ZZZ3
