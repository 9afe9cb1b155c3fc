"""Exact relations -- signed sums of at most four terms k * P, or P itself, that are or are not the identity -- over the WHOLE curve E(Fp),
shared by tests/test_exact_relations.py (the host twin) and tests/test_exact_relations_gpu.py (k_exact_relations).  These are the equalities
the reference asserts directly (same_scalar.py:101-108, opening.py:73-76) on points it decodes unchecked, so points outside the prime-order
subgroup and 256-bit scalars taken as plain integers are legal inputs.  Plain Python on oracle/bls12_381.py and tests/codec_edge_cases.py
only -- no product code -- and deterministic.

Every point of the fixture is a * G + b * T3 + c * t11 for the generator G, T3 of order 3 and t11 of order 11, built by the oracle from
its residues (a mod r, b mod 3, c mod 11).  The EXPECTED VERDICT is the oracle's own point arithmetic on the points themselves (integer
double-and-add per term, then the signed sum); the residues serve only to build inputs and to replay, in plain ints, the route the device
kernel takes through one relation -- one 4-bit-window ladder shared by the scalar terms (four doublings, then per term the table entry
d * (+-P) where the digit d is not zero), then the "one" terms -- and so which exceptional additions it meets.  cases() fails when an
event of REQUIRED_EVENTS never occurs, when the replay's verdict differs from the oracle's, or when a category lacks one of the two
verdicts."""
import functools
import random

import codec_edge_cases as E
from oracle import bls12_381 as O

R = O.R
ONE = "one"                                        # the scalar of a term that is the point itself
TERMS = 4
NEG, ONE_MARK, NONE_MARK = 0x80000000, 0x7FFFFFFF, 0xFFFFFFFF      # the record format (include/curdle_g1.h: CG1_EXACT_*)
LADDER_EVENTS = ("acc == T", "acc == -T", "identity acc revived", "identity entry, acc finite", "identity entry, acc identity")
SKIP_EVENTS = ("zero scalar", "identity base")
ONE_EVENTS = ("one: acc == P", "one: acc == -P", "one: identity acc", "one: identity operand", "one: acc finite")
REQUIRED_EVENTS = LADDER_EVENTS + SKIP_EVENTS + ONE_EVENTS
CATEGORIES = ("g1", "off 3", "off 11", "off 33", "cancelling torsion", "order 3 under r, r - 1, 2^256 - 1, 0", "same point twice",
              "same point, opposite signs", "identity operands", "one term", "two terms", "three terms", "one in every position")
MODS = (R, 3, 11)


def res_add(x, y):
    return tuple((u + v) % m for u, v, m in zip(x, y, MODS))


def res_mul(x, k):
    return tuple(u * k % m for u, m in zip(x, MODS))


ZERO = (0, 0, 0)


def replay(terms):
    """-> (events, holds) of k_exact_relations over one relation given as [(sign, k or ONE, residues) or None] * 4."""
    ev, acc, was_finite = set(), ZERO, False
    lad = []
    for t in terms:
        if t is None or t[1] == ONE:
            continue
        sign, k, res = t
        if k == 0:
            ev.add("zero scalar")
        elif res == ZERO:
            ev.add("identity base")
        else:
            lad.append((k, res_mul(res, sign)))
    if lad:
        for nib in range(63, -1, -1):
            acc = res_mul(acc, 16)                     # (every order is odd: a doubling never reaches the identity)
            for k, base in lad:
                d = (k >> (4 * nib)) & 15
                if d == 0:
                    continue
                t = res_mul(base, d)
                if t == ZERO:
                    ev.add(LADDER_EVENTS[3] if acc != ZERO else LADDER_EVENTS[4])
                    continue
                if acc == ZERO:
                    if was_finite:
                        ev.add("identity acc revived")
                elif acc == t:
                    ev.add("acc == T")
                elif res_add(acc, t) == ZERO:
                    ev.add("acc == -T")
                acc = res_add(acc, t)
                was_finite = was_finite or acc != ZERO
    for t in terms:
        if t is None or t[1] != ONE:
            continue
        p = res_mul(t[2], t[0])
        if p == ZERO:
            ev.add("one: identity operand")
            continue
        if acc == ZERO:
            ev.add("one: identity acc")
        elif acc == p:
            ev.add("one: acc == P")
        elif res_add(acc, p) == ZERO:
            ev.add("one: acc == -P")
        else:
            ev.add("one: acc finite")
        acc = res_add(acc, p)
    return ev, acc == ZERO


class Cases:
    """.points [(point or None)], .scalars [int], .relations [(category, label, [(sign, scalar index or ONE, point index) or None] * 4,
    expected verdict)], .events {event: number of relations}; .points96 / .scalars32 / .terms / .want the flat arrays a call takes."""


@functools.lru_cache(maxsize=None)
def cases():
    rng = random.Random(0xE8AC7)
    c = Cases()
    t11 = E.small_order_points(rng)[11][0]
    assert E.mul_any(E.T3, 3) is None and E.mul_any(t11, 11) is None

    # ---- points by their residues, scalars by value
    pts, pt_index, scalars, sc_index = [], {}, [], {}

    def P(a=0, b=0, c_=0):
        key = (a % R, b % 3, c_ % 11)
        if key not in pt_index:
            p = O.g1_mul(O.G1_GEN, key[0]) if key[0] else None
            p = O.g1_add(p, E.mul_any(E.T3, key[1]))
            p = O.g1_add(p, E.mul_any(t11, key[2]))
            assert p is None or O.g1_is_on_curve(p)
            pt_index[key] = len(pts)
            pts.append((p, key))
        return pt_index[key]

    def S(k):
        assert 0 <= k < 1 << 256
        if k not in sc_index:
            sc_index[k] = len(scalars)
            scalars.append(k)
        return sc_index[k]

    memo = {}

    def term_value(sign, k, pi):
        """the oracle's sign * k * points[pi], k a plain integer: double-and-add over (k mod the point's order) bits"""
        p, key = pts[pi]
        if k == ONE:
            v = p
        else:
            order = (R if key[0] else 1) * (3 if key[1] else 1) * (11 if key[2] else 1)
            mk = (pi, k % order)
            if mk not in memo:
                memo[mk] = E.mul_any(p, mk[1]) if p is not None else None
            v = memo[mk]
        return O.g1_neg(v) if sign < 0 and v is not None else v

    rels = []

    def rel(cat, label, terms):
        """terms: [(sign, k or ONE, (a, b, c)) or None]; padded to four"""
        terms = list(terms) + [None] * (TERMS - len(terms))
        assert len(terms) == TERMS
        rec, rep = [], []
        for t in terms:
            if t is None:
                rec.append(None); rep.append(None)
                continue
            sign, k, abc = t
            pi = P(*abc)
            rec.append((sign, ONE if k == ONE else S(k), pi))
            rep.append((sign, k, pts[pi][1]))
        total = None
        for t in rec:
            if t is not None:
                total = O.g1_add(total, term_value(t[0], ONE if t[1] == ONE else scalars[t[1]], t[2]))
        ev, holds = replay(rep)
        assert holds == (total is None), (cat, label)
        rels.append((cat, label, rec, total is None, ev))

    def permuted(terms, one_at):
        """the same terms with the (single) "one" term moved to position one_at"""
        i = next(j for j, t in enumerate(terms) if t is not None and t[1] == ONE)
        out = [t for j, t in enumerate(terms) if j != i]
        out.insert(one_at, terms[i])
        return out

    def draw(mod3, mod11):
        while True:
            k = rng.randrange(1 << 250, R)
            k -= k % 33
            k += next(d for d in range(33) if d % 3 == mod3 and d % 11 == mod11)
            if k < R:
                return k

    # two sets of scalars for the four-term same-scalar shape R z_k + H z_t - cm_A.T_2 - alpha T_2: "plain" (no residue mod 3 or 11 is
    # zero) and "33" (all multiples of 33, which kill a torsion component of order 3, 11 or 33)
    m = [rng.randrange(1, R) for _ in range(6)]            # discrete logarithms of the G1 points
    SETS = {"plain": (draw(1, 4), draw(2, 7), draw(1, 9)), "33": (draw(0, 0), draw(0, 0), draw(0, 0))}

    def four(which, off=None):
        """[R z_k, H z_t, -cm_A.T_2, -alpha T_2] with cm_A.T_2 = z_k R + z_t H - alpha T_2; off = {position: (b, c)} adds torsion"""
        zk, zt, al = SETS[which]
        a = [m[0], m[1], (zk * m[0] + zt * m[1] - al * m[2]) % R, m[2]]
        off = off or {}
        tor = [off.get(j, (0, 0)) for j in range(4)]
        return [(1, zk, (a[0],) + tor[0]), (1, zt, (a[1],) + tor[1]), (-1, ONE, (a[2],) + tor[2]), (-1, al, (a[3],) + tor[3])]

    def three(which, wrong=0):
        """[G_t z_t, -cm_A.T_1, -alpha T_1] with cm_A.T_1 = z_t G_t - alpha T_1 (+ wrong * G)"""
        _, zt, al = SETS[which]
        return [(1, zt, (m[3], 0, 0)), (-1, ONE, ((zt * m[3] - al * m[4] + wrong) % R, 0, 0)), (-1, al, (m[4], 0, 0))]

    # ---- relations that hold in G1 (and the same with one wrong operand), "one" in every position
    for p in range(4):
        rel("g1", f"four terms, one at {p}", permuted(four("plain"), p))
        rel("one in every position", f"four terms, one at {p}", permuted(four("33"), p))
        bad = four("plain")
        bad[p] = (bad[p][0], bad[p][1], ((bad[p][2][0] + 1) % R, 0, 0))
        rel("g1", f"four terms, operand {p} off by G", bad)
        bad33 = four("33")
        bad33[3] = (bad33[3][0], bad33[3][1], ((bad33[3][2][0] + 1) % R, 0, 0))
        rel("one in every position", f"four terms, one at {p}, alpha's operand off by G", permuted(bad33, p))
    for p in range(3):
        rel("three terms", f"same-scalar first equality, one at {p}", permuted(three("plain"), p))
        rel("three terms", f"the same off by G, one at {p}", permuted(three("plain", 1), p))
    s_, c_, k_ = draw(1, 1), draw(2, 5), m[5]
    rel("g1", "opening: s G + c k_G - A", [(1, s_, (1, 0, 0)), (1, c_, (k_, 0, 0)), (-1, ONE, ((s_ + c_ * k_) % R, 0, 0))])
    rel("g1", "opening: wrong s", [(1, s_ + 1, (1, 0, 0)), (1, c_, (k_, 0, 0)), (-1, ONE, ((s_ + c_ * k_) % R, 0, 0))])

    # ---- off by a point of order 3, 11, 33 on each term position, for "one" in every position
    for name, tor in (("3", (1, 0)), ("11", (0, 1)), ("33", (1, 1))):
        for q in range(4):                                 # (the position in the unpermuted relation; 2 is the "one" term)
            for p in range(4):
                for which in ("plain", "33"):
                    rel("off " + name, f"order {name} on operand {q}, one at {p}, {which} scalars", permuted(four(which, {q: tor}), p))

    # ---- cancelling torsion spread over two terms: operand i carries + t, operand j carries e * t with coefficient_i + e coefficient_j = 0
    for name, idx, order in (("3", 1, 3), ("11", 2, 11)):
        base = four("plain")
        coef = [(t[0] * (1 if t[1] == ONE else t[1])) % order for t in base]
        for i in range(4):
            for j in range(i + 1, 4):
                e = (-coef[i] * pow(coef[j], -1, order)) % order
                for wrong in (0, 1):
                    ee = (e + wrong) % order
                    off = {i: (1, 0) if idx == 1 else (0, 1), j: (ee, 0) if idx == 1 else (0, ee)}
                    rel("cancelling torsion", f"order {name} on operands {i} and {j}" + (", not cancelling" if wrong else ""), four("plain", off))

    # ---- a base of order 3 under r, r - 1, 2^256 - 1 and 0: the integer decides, not the value mod r
    for pos, k in enumerate((R, R - 1, (1 << 256) - 1, 0)):
        lead = [None] * (pos % 3)
        rel("order 3 under r, r - 1, 2^256 - 1, 0", f"{hex(k)[:10]} T3 alone", lead + [(1, k, (0, 1, 0))])
        rel("order 3 under r, r - 1, 2^256 - 1, 0", f"{hex(k)[:10]} T3 - (k mod 3) T3", lead + [(1, k, (0, 1, 0)), (-1, ONE, (0, k % 3, 0))])
        rel("order 3 under r, r - 1, 2^256 - 1, 0", f"{hex(k)[:10]} T3 - (k mod r mod 3) T3", lead + [(1, k, (0, 1, 0)), (-1, ONE, (0, k % R % 3, 0))])
        rel("order 3 under r, r - 1, 2^256 - 1, 0", f"{hex(k)[:10]} (T3 + G) - (k mod 3) T3 - (k mod r) G",
            lead + [(-1, ONE, (k % R, k % 3, 0)), (1, k, (1, 1, 0))])
    assert R % 3 == 1 and ((1 << 256) - 1) % 3 == 0 and ((1 << 256) - 1) % R % 3 != 0

    # ---- the same point on two terms: acc == T in mid-sum; with opposite signs: acc == -T, then the sum goes on from the identity
    k1, k2 = draw(1, 3), draw(2, 6)
    for label, abc in (("G1", (m[0], 0, 0)), ("T3", (0, 1, 0)), ("t11 + G1", (m[1], 0, 1))):
        twice = tuple(2 * v for v in abc)
        rel("same point twice", f"{label}: k P + k P - 2 k P", [(1, k1, abc), (1, k1, abc), (-1, k1, twice)])
        rel("same point twice", f"{label}: k P + k P - k P", [(1, k1, abc), (1, k1, abc), (-1, k1, abc)])
        rel("same point twice", f"{label}: P + P - 2 P", [(1, ONE, abc), (1, ONE, abc), (-1, ONE, twice)])
        rel("same point twice", f"{label}: P + P + 2 P", [(1, ONE, abc), (1, ONE, abc), (1, ONE, twice)])
        rel("same point, opposite signs", f"{label}: k P - k P + k' Q - k' Q", [(1, k1, abc), (-1, k1, abc), (1, k2, (m[3], 0, 0)), (-1, k2, (m[3], 0, 0))])
        rel("same point, opposite signs", f"{label}: k P - k P + k' Q", [(1, k1, abc), (-1, k1, abc), (1, k2, (m[3], 0, 0))])
        rel("same point, opposite signs", f"{label}: P - P", [None, (1, ONE, abc), (-1, ONE, abc)])
        rel("same point, opposite signs", f"{label}: k P - k P + Q", [(1, k1, abc), (-1, k1, abc), None, (1, ONE, (m[3], 0, 0))])

    # ---- identity operands in every position
    for p in range(4):
        for k in (SETS["plain"][0], ONE):
            for wrong in (0, 1):
                t3 = three("plain", wrong)
                t3.insert(p, (1 if p % 2 else -1, k, ZERO))
                rel("identity operands", f"identity ({'one' if k == ONE else 'scalar'}) at {p}" + (", off by G" if wrong else ""), t3)
        gone = four("plain")
        gone[p] = (gone[p][0], gone[p][1], ZERO)
        rel("identity operands", f"operand {p} replaced by the identity", gone)
    rel("identity operands", "all identity", [(1, k1, ZERO), (-1, ONE, ZERO), (1, ONE, ZERO), (-1, 0, ZERO)])
    rel("identity operands", "no term at all", [])
    rel("identity operands", "zero scalars only", [(1, 0, (m[0], 0, 0)), (-1, 0, (0, 1, 1))])
    rel("identity operands", "a zero scalar beside a live term", [(1, 0, (m[0], 0, 0)), (1, ONE, (m[1], 0, 0))])

    # ---- one, two and three terms (three: above), absent records in varying positions
    for pos, (label, t) in enumerate((("r G", (1, R, (1, 0, 0))), ("(r - 1) G", (1, R - 1, (1, 0, 0))), ("the identity", (1, ONE, ZERO)), ("G", (-1, ONE, (1, 0, 0))),
                                      ("0 G", (1, 0, (1, 0, 0))), ("33 (T3 + t11)", (-1, 33, (0, 1, 1))), ("11 (T3 + t11)", (1, 11, (0, 1, 1))),
                                      ("2 r (T3 + G)", (1, 2 * R, (m[0], 1, 0))), ("48 T3: digits 3 0", (1, 48, (0, 1, 0))),
                                      ("0x13 T3: an identity entry after a finite one", (1, 0x13, (0, 1, 0))))):
        rel("one term", label, [None] * (pos % 4) + [t])
    for pos, (label, ts) in enumerate((("k P - kP", [(1, k1, (m[0], 0, 0)), (-1, ONE, (k1 * m[0], 0, 0))]), ("k P - (k + 1) P", [(1, k1, (m[0], 0, 0)), (-1, ONE, (k1 * m[0] + m[0], 0, 0))]),
                                       ("P - P", [(1, ONE, (m[2], 1, 0)), (-1, ONE, (m[2], 1, 0))]), ("P + P", [(1, ONE, (m[2], 1, 0)), (1, ONE, (m[2], 1, 0))]),
                                       ("k T3 + k' T3", [(1, 4, (0, 1, 0)), (1, 0x20, (0, 1, 0))]), ("k T3 - k' T3", [(1, 4, (0, 1, 0)), (-1, 0x20, (0, 1, 0))]),
                                       ("0x31 T3 + 0x10 t11", [(1, 0x31, (0, 1, 0)), (1, 0x10, (0, 0, 1))]))):
        rel("two terms", label, [None] * (pos % 3) + ts)

    # ---- what the list reaches
    c.events = {}
    for _, _, _, _, ev in rels:
        for e in ev:
            c.events[e] = c.events.get(e, 0) + 1
    missing = [e for e in REQUIRED_EVENTS if not c.events.get(e)]
    assert not missing, f"no relation drives the sum into: {missing}"
    for cat in CATEGORIES:
        verdicts = {r[3] for r in rels if r[0] == cat}
        assert verdicts == {True, False}, (cat, verdicts)
    for cat in ("off 3", "off 11", "off 33"):      # both verdicts on each operand (the "one" operand, 2, can only fail), for "one" in every position
        for pos in range(4):
            assert {r[3] for r in rels if r[0] == cat and f"operand {pos}," in r[1]} == ({False} if pos == 2 else {True, False}), (cat, pos)
    ones = {j for r in rels for j, t in enumerate(r[2]) if t is not None and t[1] == ONE}
    assert ones == {0, 1, 2, 3}
    assert 200 <= len(rels) <= 300, len(rels)

    c.points = [p for p, _ in pts]
    c.scalars = scalars
    c.relations = [r[:4] for r in rels]
    c.points96 = b"".join(E.raw96(p) if p is not None else bytes(96) for p in c.points)
    c.scalars32 = b"".join(k.to_bytes(32, "little") for k in scalars)
    c.want = [r[3] for r in rels]
    c.terms = pack_terms(r[2] for r in rels)
    return c


def pack_terms(relations):
    """[[(sign, scalar index or ONE, point index) or None] * 4] -> the records of the C ABI, little-endian uint32 pairs"""
    out = bytearray()
    for rec in relations:
        assert len(rec) == TERMS
        for t in rec:
            if t is None:
                out += NONE_MARK.to_bytes(4, "little") + (0).to_bytes(4, "little")
            else:
                sign, k, pi = t
                word = (ONE_MARK if k == ONE else k) | (NEG if sign < 0 else 0)
                out += pi.to_bytes(4, "little") + word.to_bytes(4, "little")
    return bytes(out)
