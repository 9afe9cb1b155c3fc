"""Scalar multiplications, point sums and MSM inputs over the WHOLE curve E(Fp), shared by tests/test_curve_mul.py (host) and
tests/test_curve_mul_gpu.py (device).  The reference decodes points unchecked (util.py:35-36), so points outside the prime-order
subgroup are legal inputs of `G1Point * Scalar`, the folds and the MSMs: bases of order 3, 11, 10177, 859267, 52437899 and 33, their
sums with points of G1, the identity, and 256-bit scalars taken as plain integers (for a base outside G1 the value itself decides the
result, not the value mod r).  Plain Python on oracle/bls12_381.py and tests/codec_edge_cases.py only -- no product code -- and
deterministic; every expected value is the oracle's integer double-and-add.

Which exceptional additions the case list drives a ladder into is ASSERTED, not hoped for: ladder_events() replays the binary ladder
(k_batch_mul: double, add on a set bit), the radix-4 ladder (k_batch_mul_quad: two doublings, add d P from {P, 2P, 3P}) and the radix-16
ladder (k_batch_mul_row: four doublings, add d P from {P .. 15P}) over residues mod the base's order, and cases() fails if an event of
REQUIRED_EVENTS never occurs; tree_events() does the same for the lane sums and the 64-lane shuffle tree of k_batch_sum."""
import functools
import random

import codec_edge_cases as E
from oracle import bls12_381 as O

R = O.R
T3 = E.T3
ADDENDS = ("identity", "+sB", "-sB", "unrelated")          # A of the fold form A + s B (beside "none": no addend array at all)
# per ladder: the doubling branch, the cancellation, an addition into an identity accumulator that had been finite; from radix 4 on
# a selected table entry that is itself the identity, met with a finite and with an identity accumulator
LADDER_EVENTS = ("acc == T", "acc == -T", "identity acc revived")
TABLE_EVENTS = ("identity entry, acc finite", "identity entry, acc identity")
REQUIRED_EVENTS = {1: LADDER_EVENTS, 2: LADDER_EVENTS + TABLE_EVENTS, 4: LADDER_EVENTS + TABLE_EVENTS}     # by bits per digit
TREE_EVENTS = ("lane: acc == P", "lane: acc == -P", "lane: identity acc revived", "lane: identity entry",
               "tree: acc == o", "tree: acc == -o", "tree: identity acc, finite o", "tree: finite acc, identity o", "tree: identity both")


def add(a, b):
    return O.g1_add(a, b)


def neg(a):
    return O.g1_neg(a)


def s32(k):
    assert 0 <= k < 1 << 256
    return k.to_bytes(32, "little")


def ladder_events(order, k, w):
    """-> (events, the final multiple mod order) of the MSB-first ladder with w bits per digit over a base of that order (> 1): before
    each digit w doublings, then the table entry d * B is added where the digit d is not zero.  Leading zero digits leave the identity
    accumulator alone, skipped (k_batch_mul) or not.  The order is odd, so a doubling never reaches the identity."""
    assert order > 1 and order % 2 == 1 and 256 % w == 0
    ev, acc, was_finite = set(), 0, False                 # acc: the accumulator as a multiple of B mod order; 0 = the identity
    for i in range(256 // w - 1, -1, -1):
        acc = (acc << w) % order
        d = (k >> (w * i)) & ((1 << w) - 1)
        if d == 0:
            continue
        t = d % order
        if t == 0:
            ev.add(TABLE_EVENTS[0] if acc else TABLE_EVENTS[1])
            continue
        if acc == 0:
            if was_finite:
                ev.add("identity acc revived")
        elif acc == t:
            ev.add("acc == T")
        elif (acc + t) % order == 0:
            ev.add("acc == -T")
        acc = (acc + t) % order
        was_finite = was_finite or acc != 0
    return ev, acc


def tree_events(pts):
    """-> (events, the sum) of k_batch_sum over one group, replayed on oracle points: lane l adds the entries l, l + 64, ... one after the
    other (identity records skipped), then for delta = 32 .. 1 lane l < delta adds lane l + delta's partial sum to its own."""
    ev, lanes = set(), []
    for l in range(64):
        acc, was_finite = None, False
        for p in pts[l::64]:
            if p is None:
                ev.add("lane: identity entry")
                continue
            if acc is None:
                if was_finite:
                    ev.add("lane: identity acc revived")
            elif acc == p:
                ev.add("lane: acc == P")
            elif acc == neg(p):
                ev.add("lane: acc == -P")
            acc = add(acc, p)
            was_finite = was_finite or acc is not None
        lanes.append(acc)
    delta = 32
    while delta:
        for l in range(delta):
            a, o = lanes[l], lanes[l + delta]
            if a is None or o is None:
                ev.add("tree: identity both" if a is None and o is None else "tree: identity acc, finite o" if a is None else "tree: finite acc, identity o")
            elif a == o:
                ev.add("tree: acc == o")
            elif a == neg(o):
                ev.add("tree: acc == -o")
            lanes[l] = add(a, o)
        delta >>= 1
    return ev, lanes[0]


def index_shapes(c):
    """[(first base, nbase, first scalar, nscalars, n)] for out[i] = scalars[i % nscalars] * bases[i % nbase] over the fixture's lists:
    one base under every scalar (t3, order 11), every base under one scalar (7, 13: the radix-4 digits 1 3 and 3 1), and counts that do
    not divide n."""
    nb, ns = len(c.bases), len(c.scalars)
    i7, i13 = c.scalars.index(7), c.scalars.index(13)
    return [(3, 1, 0, ns, ns), (5, 1, 0, ns, ns), (0, nb, i7, 1, nb), (0, nb, i13, 1, nb), (0, nb, 0, ns, 129), (1, nb - 1, 2, ns - 2, 65)]


class Cases:
    def want(self, b, k):
        """k * bases[b] for the plain integer k: (k mod order) * B by the oracle's double-and-add, remembered."""
        _, pt, order = self.bases[b]
        key = (b, k % order)
        if key not in self._memo:
            self._memo[key] = E.mul_any(pt, key[1])
        return self._memo[key]


@functools.lru_cache(maxsize=None)
def cases():
    """The whole fixture:
    .bases     [(label, point or None, order)]  the identity first; every order checked against the oracle
    .scalars   the 256-bit integers
    .unrelated a point of G1 that is no base
    .pairs     [(b, k)]  every base with every scalar
    .mul       [(b, k, addend kind or "none", addend point, expected point)]  every pair without an addend, and once more with one of ADDENDS
    .events    {bits per digit: {event: number of pairs that reach it}}
    .sums      [(label, [points], expected sum)]  the groups for the segmented point sum
    .sum_events  {event: number of groups}
    .msm       ([points], [scalars], expected sum): ~300 terms over the bases, repeats and both signs of each
    .lincomb   ([bases], offsets, term_base, scalars, [expected]): map, fold and four-to-six-term combinations, negated-base bit included
    """
    rng = random.Random(0xC7A5E)
    c = Cases()
    c._memo = {}
    small = E.small_order_points(rng)
    g = [O.g1_mul(O.G1_GEN, rng.randrange(1, R)) for _ in range(3)]
    t11 = small[11][0]
    c.unrelated = g[2]
    c.bases = [("identity", None, 1), ("g1 a", g[0], R), ("g1 b", g[1], R), ("t3", T3, 3), ("-t3", neg(T3), 3)]
    c.bases += [(f"order {ell}", small[ell][0], ell) for ell in E.SMALL_PRIMES]
    c.bases += [("t3 + g1", add(T3, g[0]), 3 * R), ("order 11 + g1", add(t11, g[1]), 11 * R), ("t3 + order 11", add(T3, t11), 33)]
    prime_factors = lambda m: [q for q in (3, 11, 10177, 859267, 52437899, R) if m % q == 0]
    for label, pt, order in c.bases:                       # each base carries its order: order * B = 0 and (order / q) * B != 0
        assert O.g1_is_on_curve(pt) and E.mul_any(pt, order) is None, label
        assert all(E.mul_any(pt, order // q) is not None for q in prime_factors(order)), label

    pat = lambda byte: int.from_bytes(bytes([byte]) * 32, "little")
    sc = list(range(9)) + [12, 13, 15] + [pat(b) for b in (0x55, 0xAA, 0xFF, 0x33, 0xCC, 0x77)]
    for k in (31, 32, 33, 63, 64, 65, 127, 128, 254, 255):
        sc += [1 << k, (1 << k) - 1]
    sc += [R - 1, R, R + 1, 2 * R]
    for m in (3, 11, 33, 10177, 859267, 52437899):         # 200-bit multiples of each small order, and their neighbours
        for _ in range(2):
            q = rng.getrandbits(200) | (1 << 199)
            q -= q % m
            sc += [q - 1, q, q + 1]
    sc += [rng.getrandbits(256) | (1 << 255) for _ in range(3)] + [rng.getrandbits(255) | (1 << 254) for _ in range(3)]
    c.scalars = list(dict.fromkeys(sc))
    assert all(0 <= k < 1 << 256 for k in c.scalars) and pat(0xFF) == (1 << 256) - 1
    c.pairs = [(b, k) for b in range(len(c.bases)) for k in c.scalars]

    # ---- (k mod order) * B is k * B: the oracle's full 256-bit double-and-add on a seeded sample
    sample = rng.sample([(b, k) for b, k in c.pairs if k >= c.bases[b][2]], 48)
    assert len({b for b, _ in sample}) >= 8
    for b, k in sample:
        assert E.mul_any(c.bases[b][1], k) == c.want(b, k), (c.bases[b][0], hex(k))

    # ---- what the ladders meet on these pairs
    c.events = {}
    for w, required in REQUIRED_EVENTS.items():
        count = {}
        for b, k in c.pairs:
            order = c.bases[b][2]
            if order == 1:
                continue
            ev, end = ladder_events(order, k, w)
            assert end == k % order
            for e in ev:
                count[e] = count.get(e, 0) + 1
        missing = [e for e in required if not count.get(e)]
        assert not missing, f"no (base, scalar) pair drives the {w}-bit ladder into: {missing}"
        c.events[w] = count

    # ---- s * B and A + s * B
    c.mul = []
    for b, k in c.pairs:
        c.mul.append((b, k, "none", None, c.want(b, k)))
    for i, (b, k) in enumerate(c.pairs):
        sb = c.want(b, k)
        kind = ADDENDS[(i + i // len(c.scalars)) % 4]      # (every base meets every kind, every scalar meets several)
        a = {"identity": None, "+sB": sb, "-sB": neg(sb), "unrelated": c.unrelated}[kind]
        c.mul.append((b, k, kind, a, add(a, sb)))
    for kind in ADDENDS:                                   # the final addition doubles, cancels, meets an identity on either side
        hit = [m for m in c.mul if m[2] == kind]
        assert any(c.want(m[0], m[1]) is not None for m in hit) and any(c.want(m[0], m[1]) is None for m in hit), kind
        assert all((m[4] is None) == (kind == "-sB") for m in hit if c.want(m[0], m[1]) is not None), kind

    # ---- groups for the segmented sum
    p, q = g[0], g[1]
    menu = [None, T3, neg(T3), t11, neg(t11), p, neg(p), q, small[10177][0]]
    groups = [("t3 x 2", [T3] * 2), ("t3 x 3", [T3] * 3), ("t3 x 64", [T3] * 64), ("p - p + q", [p, neg(p), q]), ("empty", [])]
    for n in (1, 63, 64, 65, 129):
        pts = [menu[rng.randrange(len(menu))] for _ in range(n)]
        if n >= 65:
            pts[0], pts[64] = p, neg(p)                    # lane 0's own sum is the identity when the tree starts
            pts[33], pts[1] = T3, T3                       # (lane 1 and lane 33 hold equal sums unless index 65 / 97 says otherwise)
        if n == 129:
            pts[128], pts[32] = q, None                    # lane 0: p - p + q, an identity revived; lane 32: an identity record
            pts[2], pts[66] = t11, t11                     # lane 2: a doubling
        groups.append((f"mixed x {n}", pts))
    groups.append(("t3 x 129", [T3] * 129))                # lane 0: t3 + t3 + t3; the tree adds equal sums at every level
    groups.append(("identities x 65", [None] * 65))
    c.sums, c.sum_events = [], {}
    for label, pts in groups:
        ev, total = tree_events(pts)
        ref = None
        for pt in pts:
            ref = add(ref, pt)
        assert total == ref, label
        c.sums.append((label, pts, ref))
        for e in ev:
            c.sum_events[e] = c.sum_events.get(e, 0) + 1
    missing = [e for e in TREE_EVENTS if not c.sum_events.get(e)]
    assert not missing, f"no group drives k_batch_sum into: {missing}"
    assert {len(pts) for _, pts, _ in c.sums} >= {0, 1, 2, 3, 63, 64, 65, 129}

    # ---- one MSM over the bases: repeats and both signs of each, scalars below 2^255 as plain integers
    special = [k for k in c.scalars if k < 1 << 255]
    pts, ks, coef = [], [], [0] * len(c.bases)
    for i in range(300):
        b = i % len(c.bases) if i < 4 * len(c.bases) else rng.randrange(len(c.bases))
        sign = -1 if (i // len(c.bases)) % 2 else 1         # (the first rounds: every base with both signs, twice)
        k = special[rng.randrange(len(special))] if i % 3 == 0 else rng.getrandbits(255)
        pt = c.bases[b][1]
        pts.append(pt if sign > 0 else neg(pt))
        ks.append(k)
        coef[b] += sign * k
    total = None
    for b, (_, pt, order) in enumerate(c.bases):
        total = add(total, E.mul_any(pt, coef[b] % order))
    for i in rng.sample(range(300), 12):                   # (the per-base bookkeeping against the terms themselves, on a sample)
        b = next(b for b, (_, pt, _) in enumerate(c.bases) if pts[i] in (pt, neg(pt)))
        assert E.mul_any(pts[i], ks[i]) == (c.want(b, ks[i]) if pts[i] == c.bases[b][1] else neg(c.want(b, ks[i])))
    c.msm = (pts, ks, total)

    # ---- linear combinations over shared bases: every s * B and s * (-B) by the negated-base bit, every A + s * B (each third
    # with the bit), and combinations of four to six weighted terms
    lb = [pt for _, pt, _ in c.bases]
    offsets, tb, ls, want = [0], [], [], []
    for i, (b, k, kind, a, w) in enumerate(c.mul):
        for flip in ((False, True) if kind == "none" else (i % 3 == 1,)):
            if kind != "none":
                tb.append(len(lb)); ls.append(1); lb.append(a)
            tb.append(b | (0x80000000 if flip else 0)); ls.append(k)
            want.append(add(a, neg(c.want(b, k))) if flip else w)
            offsets.append(len(tb))
    for _ in range(60):
        acc = None
        for _ in range(rng.randrange(4, 7)):
            b, k, flip = rng.randrange(len(c.bases)), c.scalars[rng.randrange(9, len(c.scalars))], rng.random() < 0.3
            tb.append(b | (0x80000000 if flip else 0)); ls.append(k)
            acc = add(acc, neg(c.want(b, k)) if flip else c.want(b, k))
        want.append(acc)
        offsets.append(len(tb))
    c.lincomb = (lb, offsets, tb, ls, want)
    return c
