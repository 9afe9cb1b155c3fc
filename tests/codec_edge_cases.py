"""Adversarial wire encodings and curve points shared by tests/test_codec_edges.py (host) and tests/test_codec_edges_gpu.py (device):
points whose y lies next to (p-1)/2 and x values next to p AT EVERY 32-BIT WORD of the word-by-word comparisons, the flag patterns, and
a list of points for the subgroup tests (small-order points of every prime factor of the cofactor, their sums with G1 points, points of
full order).  Plain Python on oracle/bls12_381.py only -- no product code -- and deterministic; every expected value (status class,
decoded point, encoding, subgroup flag) is the oracle's.  cases() builds everything once per process."""
import functools
import random

from oracle import bls12_381 as O

P = O.P
H = (P - 1) // 2
M32 = 0xFFFFFFFF
MAX_STEPS = 64                                    # a search that needs more is a bug in the builder: fail loudly
OK, ENCODING, NOT_ON_CURVE, NOT_IN_SUBGROUP = "ok", "encoding", "not_on_curve", "not_in_subgroup"
T3 = (0, 2)                                       # order 3 (tests/golden/torsion_vectors.json "t3")
ZM1 = 0xd201000000010001                          # |z| + 1 = 3 * 11 * 10177 * 859267 * 52437899; the cofactor is (z - 1)^2 / 3
H_COF = ZM1 * ZM1 // 3
SMALL_PRIMES = (11, 10177, 859267, 52437899)
assert ZM1 == 3 * 11 * 10177 * 859267 * 52437899 and H_COF * O.R == P + 1 - (-(ZM1 - 1) + 1)    # #E(Fp) = p + 1 - t, t = z + 1


def words(v):
    return [(v >> (32 * i)) & M32 for i in range(12)]


# ------------------------------------------------------------------ cube roots mod p  (p = 1 mod 9, p - 1 = 9 t, 3 does not divide t)
_T = (P - 1) // 9
assert (P - 1) % 9 == 0 and _T % 3 != 0
_G = next(g for g in range(2, 50) if pow(g, (P - 1) // 3, P) != 1)          # a non-cube
_C3 = pow(_G, 3 * _T, P)                                                    # g^t has order 9, this its cube: order 3
_INV3_T = pow(3, -1, _T)


def is_cube(a):
    return a % P == 0 or pow(a, (P - 1) // 3, P) == 1


def cube_root(a):
    """One r with r^3 == a (mod p) for a cube a.  a^t lies in the order-3 group {1, c, c^2}, c = g^3t: with a^t = c^k the element
    a' = a g^(-3k) has a'^t = 1, lies in the subgroup of order t where cubing is a bijection, so a'^(1/3 mod t) is its root; times g^k."""
    a %= P
    if a == 0:
        return 0
    at = pow(a, _T, P)
    k = next(k for k in range(3) if pow(_C3, k, P) == at)
    a1 = a * pow(_G, -3 * k, P) % P
    r = pow(a1, _INV3_T, P) * pow(_G, k, P) % P
    assert pow(r, 3, P) == a
    return r


# ------------------------------------------------------------------ group helpers (integers taken as they are: the points may lie outside G1)
def mul_any(pt, k):
    """k * pt WITHOUT reducing k mod r."""
    acc, base = O.JAC_INF, O.jac_from_affine(pt)
    for bit in bin(k)[2:] if k else "":
        acc = O.jac_double(acc)
        if bit == "1":
            acc = O.jac_add(acc, base)
    return O.jac_to_affine(acc)


@functools.lru_cache(maxsize=None)
def in_g1(pt):
    """O.g1_in_subgroup, remembered (a quarter of a thousand doublings in Python each)."""
    return O.g1_in_subgroup(pt)


def raw96(pt):
    return bytes(96) if pt is None else pt[0].to_bytes(48, "little") + pt[1].to_bytes(48, "little")


def enc_x(x, flags):
    """48 bytes: x (< 2^381) big-endian under the three flag bits."""
    assert 0 <= x < 1 << 381 and flags & 0x1F == 0
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


_MESSAGES = {"compression flag not set": ENCODING, "x not canonical": ENCODING, "x is not on the curve": NOT_ON_CURVE,
             "point not in the prime-order subgroup": NOT_IN_SUBGROUP}


def expect_decode(enc, check):
    """(status class, affine96) as O.g1_decompress decides; a refused encoding leaves the all-zero record."""
    try:
        pt = O.g1_decompress(enc, False)
    except ValueError as e:
        return _MESSAGES[str(e)], bytes(96)
    if check and not in_g1(pt):                   # (O.g1_decompress(enc, True) is this decoding followed by O.g1_in_subgroup)
        return NOT_IN_SUBGROUP, bytes(96)
    return OK, raw96(pt)


# ------------------------------------------------------------------ the sign boundary: y next to (p-1)/2 at every word
def boundary_points(inner=False):
    """[(j, side, (x, y))]: for every word index j and side the curve point whose y is nearest to h +- 2^(32 j) on the far side of it
    (j = 0: nearest above h, and nearest at or below h): the words of y above j equal those of h, and word j decides.
    inner: the nearest on the NEAR side instead (j >= 1): word j still differs from h's by one and decides, but the words below it
    point the other way -- a comparison that took word j for equal (a constant off by one there) would go on and decide wrongly."""
    out = []
    hw = words(H)
    for j in range(1 if inner else 0, 12):
        for side in ("above", "below"):
            step = (1 if side == "above" else -1) * (-1 if inner else 1)
            start = H + (1 << (32 * j)) if side == "above" else H - (1 << (32 * j))
            if inner:
                start += step
            if j == 0:
                start = H + 1 if side == "above" else H
            for d in range(MAX_STEPS + 1):
                y = start + step * d
                if is_cube(y * y - 4):
                    break
            else:
                raise AssertionError(f"no curve point within {MAX_STEPS} of the boundary at word {j} ({side})")
            x = cube_root(y * y - 4)
            pt = (x, y)
            yw = words(y)
            assert O.g1_is_on_curve(pt) and yw[j + 1:] == hw[j + 1:] and yw[j] != hw[j], (j, side)
            assert (y > H) == (side == "above") and (yw[j] > hw[j]) == (side == "above")
            low = (1 << (32 * j)) - 1
            assert not inner or (abs(yw[j] - hw[j]) == 1 and (y & low != H & low) and ((y & low) < (H & low)) == (side == "above"))
            out.append((j, side, pt))
    return out


# ------------------------------------------------------------------ the range check: x next to p at every word
def x_range_cases():
    """-> (refused x >= p, [(j, x)] accepted with x^3 + 4 a square, [(j, x)] with x^3 + 4 a non-square); every x keeps p's words above j,
    and word j decides.  Then the same two from the near side (j >= 1): x = p + 2^(32 j) - 1, refused although every word below j is
    smaller than p's, and the nearest x >= p - 2^(32 j) + 1 on the curve, accepted although the words below j are larger than p's."""
    pw = words(P)
    over, square, non_square, over_inner, square_inner = [], [], [], [], []
    for j in range(12):
        x = P + (1 << (32 * j))
        assert x < 1 << 381 and words(x)[j + 1:] == pw[j + 1:] and words(x)[j] > pw[j]
        over.append((j, x))
        found = {}
        for d in range(MAX_STEPS + 1):
            x = P - (1 << (32 * j)) - d
            found.setdefault(O.fp_sqrt((x ** 3 + 4) % P) is not None, x)
            if len(found) == 2:
                break
        else:
            raise AssertionError(f"no square and non-square x^3 + 4 within {MAX_STEPS} below p - 2^(32*{j})")
        for x in found.values():
            assert words(x)[j + 1:] == pw[j + 1:] and words(x)[j] < pw[j]
        square.append((j, found[True]))
        non_square.append((j, found[False]))
        if j == 0:
            continue
        low = (1 << (32 * j)) - 1
        x = P + (1 << (32 * j)) - 1
        assert words(x)[j + 1:] == pw[j + 1:] and words(x)[j] == pw[j] + 1 and (x & low) < (P & low)
        over_inner.append((j, x))
        for d in range(1, MAX_STEPS + 2):
            x = P - (1 << (32 * j)) + d
            if O.fp_sqrt((x ** 3 + 4) % P) is not None:
                break
        else:
            raise AssertionError(f"no square x^3 + 4 within {MAX_STEPS} above p - 2^(32*{j})")
        assert words(x)[j + 1:] == pw[j + 1:] and words(x)[j] == pw[j] - 1 and (x & low) > (P & low)
        square_inner.append((j, x))
    return over, square, non_square, over_inner, square_inner


# ------------------------------------------------------------------ which exceptional additions a point of small order reaches
Z_ABS = 0xd201000000010000


def chain_events(order):
    """Replay of the device subgroup tests' two passes  Q = [|z|] P,  acc = [|z|] Q  (double, then add the pass's base where |z| has a
    one, from bit 62 down) over multiples of a point P of that order: the set of (pass, event) the additions run into -- "P+P" (equal
    operands: the doubling branch), "P-P" (opposite operands) and "inf" (an identity operand)."""
    ev = set()
    for nr, base in ((1, 1 % order), (2, None)):
        if nr == 2:
            base = acc
        acc = base
        for bit in range(62, -1, -1):
            acc = 2 * acc % order
            if (Z_ABS >> bit) & 1:
                ev.add((nr, "inf" if acc == 0 or base == 0 else "P+P" if acc == base else "P-P" if (acc + base) % order == 0 else "add"))
                acc = (acc + base) % order
    return ev


# ------------------------------------------------------------------ points of small order (shared with tests/curve_mul_cases.py)
def curve_point(rng):
    """A point of E(Fp) drawn with rng: almost surely of full order h * r, outside G1."""
    while True:
        x = rng.randrange(P)
        y = O.fp_sqrt((x * x * x + 4) % P)
        if y is not None:
            return (x, y if rng.randrange(2) else P - y)


def small_order_points(rng):
    """{ell: [t, t']} for every ell of SMALL_PRIMES: two different points of order ell, drawn with rng (order 3 is T3 itself)."""
    small = {}
    for ell in SMALL_PRIMES:
        # the cofactor group is Z/((z-1)/3) x Z/(z-1): its ell-part is (Z/ell)^2, so R * (h / ell^2) maps a curve point into it
        got = []
        for _ in range(MAX_STEPS):
            t = mul_any(curve_point(rng), O.R * (H_COF // (ell * ell)))
            if t is None:
                continue
            assert O.g1_is_on_curve(t) and mul_any(t, ell) is None
            # independent of the first: checked for ell = 11; for the larger ell a second random element of (Z/ell)^2 lies in the
            # first's span with probability 1 / ell < 10^-4, and a dependent pair would only repeat a case, not weaken one
            if got and ell == 11 and any(mul_any(got[0], k) == t for k in range(ell)):
                continue
            got.append(t)
            if len(got) == 2:
                break
        assert len(got) == 2 and got[0] != got[1], ell
        small[ell] = got
    return small


# ------------------------------------------------------------------ everything, once
class Cases:
    pass


@functools.lru_cache(maxsize=None)
def cases():
    """The whole fixture:
    .boundary      [(j, side, pt)]  24 word/side pairs
    .boundary_pts  the 48 points: each of those and its negative (on the curve, none in G1)
    .inner, .inner_pts  the same from the near side of h +- 2^(32 j), j >= 1: 22 pairs, 44 points
    .encodings     [(class label, 48 bytes)]  every wire case: boundary points, x-range cases, x = 0 / p - 1 / p / 2^381 - 1, flag cases
    .valid_points  the points behind the encodings that decode to a point (for the compress direction)
    .g1            6 points of G1
    .fillers       170 further points of G1 (a chain of additions: cheap), for interleaving and padding
    .subgroup      [(class label, pt)]  the list for the subgroup tests; expected flag = in_g1(pt)
    """
    rng = random.Random(0xC0DEC)
    c = Cases()
    c.boundary = boundary_points()
    c.boundary_pts = []
    for _, _, pt in c.boundary:
        c.boundary_pts += [pt, O.g1_neg(pt)]
    assert len(c.boundary_pts) == 48
    # (h + 1 + d and h - d are negatives of each other, so the negative of an "above" point may BE the "below" point of its word: the
    # 48 hold fewer distinct points, and lists that must not repeat a case take them once)
    c.boundary_distinct = list(dict.fromkeys(c.boundary_pts))
    c.inner = boundary_points(inner=True)
    c.inner_pts = []
    for _, _, pt in c.inner:
        c.inner_pts += [pt, O.g1_neg(pt)]
    assert len(c.inner_pts) == 44           # (h - 2^(32 j) + 1 is the negative of h + 2^(32 j): some are boundary points already)
    assert all(O.g1_is_on_curve(p) and not in_g1(p) for p in c.boundary_pts + c.inner_pts)

    enc = [("boundary", O.g1_compress(p)) for p in c.boundary_distinct] + [("boundary inner", O.g1_compress(p)) for p in dict.fromkeys(c.inner_pts)]
    over, square, non_square, over_inner, square_inner = x_range_cases()
    c.x_over, c.x_square, c.x_non_square, c.x_over_inner, c.x_square_inner = over, square, non_square, over_inner, square_inner
    for _, x in over_inner:
        enc += [("x>=p", enc_x(x, 0x80 if x & 2 else 0xA0))]
    for _, x in square_inner:
        enc += [("x<p square", enc_x(x, 0x80)), ("x<p square", enc_x(x, 0xA0))]
    for _, x in over:
        enc += [("x>=p", enc_x(x, 0x80)), ("x>=p", enc_x(x, 0xA0))]
    for _, x in square:
        enc += [("x<p square", enc_x(x, 0x80)), ("x<p square", enc_x(x, 0xA0))]
    for _, x in non_square:
        enc += [("x<p non-square", enc_x(x, 0x80 if x & 1 else 0xA0))]
    enc += [("x=0", enc_x(0, 0x80)), ("x=0", enc_x(0, 0xA0)), ("x=p-1", enc_x(P - 1, 0x80)), ("x=p-1", enc_x(P - 1, 0xA0)),
            ("x=p", enc_x(P, 0x80)), ("x=p", enc_x(P, 0xA0)), ("x=2^381-1", enc_x((1 << 381) - 1, 0x80))]
    vx = square[3][1]                                                        # a valid x for the flag cases
    enc += [("flag clear", enc_x(vx, 0x00)), ("flag clear", enc_x(vx, 0x20)), ("flag clear", enc_x(vx, 0x40)), ("flag clear", bytes(48)),
            ("infinity+sign", enc_x(0, 0xE0)), ("infinity+junk", enc_x(vx, 0xC0)), ("infinity+junk", enc_x(vx, 0xE0)),
            ("infinity+junk", enc_x((1 << 381) - 1, 0xC0)), ("infinity+junk", enc_x(1, 0xC0)), ("infinity", enc_x(0, 0xC0))]
    c.encodings = list({e: (label, e) for label, e in reversed(enc)}.values())[::-1]       # (x = p - 1 is also word 0's nearest x: once)
    assert len(set(e for _, e in c.encodings)) == len(c.encodings)

    c.valid_points = []
    for _, e in c.encodings:
        st, raw = expect_decode(e, False)
        if st == OK and raw != bytes(96):
            c.valid_points.append((int.from_bytes(raw[:48], "little"), int.from_bytes(raw[48:], "little")))
    assert set(c.boundary_pts + c.inner_pts) <= set(c.valid_points) and {T3, O.g1_neg(T3)} <= set(c.valid_points)
    assert all(O.g1_is_on_curve(p) for p in c.valid_points)

    # ---- points for the subgroup tests
    c.g1 = [O.g1_mul(O.G1_GEN, rng.randrange(1, O.R)) for _ in range(6)]
    c.fillers = [O.g1_add(c.g1[1], c.g1[2])]
    while len(c.fillers) < 170:
        c.fillers.append(O.g1_add(c.fillers[-1], c.g1[3]))
    wild = [curve_point(rng) for _ in range(6)]
    sub = [("g1", p) for p in c.g1] + [("identity", None)] + [("wild", p) for p in wild] + [("t3", T3)]
    small = small_order_points(rng)
    for ell in SMALL_PRIMES:
        sub += [(f"order {ell}", t) for t in small[ell]]
    i = 0
    for ell in SMALL_PRIMES:
        for t in small[ell]:
            sub.append((f"order {ell} + g1", O.g1_add(t, c.g1[i % 6])))
            i += 1
    sub.append(("t3 + g1", O.g1_add(T3, c.g1[0])))
    sub.append(("t3 + order 11", O.g1_add(T3, small[11][0])))
    sub.append(("r * wild", mul_any(wild[1], O.R)))
    sub.append(("h * wild", mul_any(wild[2], H_COF)))
    sub += [("boundary", p) for p in c.boundary_distinct]
    assert all(O.g1_is_on_curve(p) for _, p in sub)
    inside = {"g1", "identity", "h * wild"}
    for label in dict(sub):
        flags = [in_g1(p) for lab, p in sub if lab == label]
        assert all(flags) if label in inside else not any(flags), label
    # the pure small-order points are what reaches the out-of-line paths of quad_add / row_add: order 3 cancels and meets the identity,
    # order 11 meets EQUAL operands in both passes (with a G1 part added the multiples never coincide, and neither do those of larger order)
    assert {(1, "P-P"), (1, "inf")} <= chain_events(3) and {(1, "P+P"), (2, "P+P")} <= chain_events(11)
    c.subgroup = sub
    c.small = small
    return c
