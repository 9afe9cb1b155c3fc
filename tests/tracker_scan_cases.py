"""Inputs and expected bitmaps of the tracker scan -- bit (i, j) = [k_j * r_G_i == k_r_G_i] over unchecked decodings (util.py:35-36) --
shared by tests/test_tracker_scan.py (the host twin) and tests/test_tracker_scan_gpu.py (the device).  Plain Python on
oracle/bls12_381.py, oracle/c_oracle.py, tests/codec_edge_cases.py and tests/curve_mul_cases.py only -- no product code -- and
deterministic.  Every expected bit is the oracle's integer double-and-add (c_oracle.scalar_mul: all 256 bits of the scalar, no
reduction mod r) held against O.g1_decompress of the tracker's k_r_G; every expected status is O.g1_decompress raising or k >= r.

Which exceptional additions the device kernel meets is ASSERTED: window_events() replays its sum -- the signed 4-bit digits of the
light tables, windows added in ASCENDING order w = 0 .. 63, the addend d * 16^w * B taken from a table (so it may itself be the
identity) -- over residues mod the base's order, as curve_mul_cases.ladder_events does for the ladders, and cases() fails if one of
EVENTS never occurs among the small-order cases."""
import functools
import json
import os
import random

import codec_edge_cases as E
import curve_mul_cases as M
from oracle import bls12_381 as O
from oracle import c_oracle as C

R = O.R
BAD_POINT, BAD_SCALAR = 2, 1
WINDOW_BITS, WINDOWS, HALF = 4, 64, 8
EVENTS = ("acc == addend", "acc == -addend", "identity entry, acc finite", "identity entry, acc identity", "identity acc revived")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def light_digits(k):
    """The signed digits d_w in [-8, 8] of k < r, least significant window first: k = sum d_w 16^w."""
    assert 0 <= k < R
    out, carry = [], 0
    for w in range(WINDOWS):
        u = ((k >> (WINDOW_BITS * w)) & 15) + carry
        carry = 1 if u > HALF else 0
        out.append(u - 16 if carry else u)
    assert carry == 0 and sum(d << (WINDOW_BITS * w) for w, d in enumerate(out)) == k
    return out


def window_events(order, k):
    """-> (events, the final multiple mod order) of the windowed sum over a base of that order (> 1): for w = 0 .. 63 the addend
    d_w * 16^w * B is added where the digit is not zero; the table entry |d_w| * 16^w * B may be the identity."""
    ev, acc, was_finite = set(), 0, False
    for w, d in enumerate(light_digits(k)):
        if d == 0:
            continue
        t = d * pow(16, w, order) % order
        if t == 0:
            ev.add(EVENTS[2] if acc else EVENTS[3])
            continue
        if acc == 0:
            if was_finite:
                ev.add(EVENTS[4])
        elif acc == t:
            ev.add(EVENTS[0])
        elif (acc + t) % order == 0:
            ev.add(EVENTS[1])
        acc = (acc + t) % order
        was_finite = was_finite or acc != 0
    return ev, acc


def from_raw96(b):
    return None if b == bytes(96) else (int.from_bytes(b[:48], "little"), int.from_bytes(b[48:], "little"))


@functools.lru_cache(maxsize=None)
def omul(pt, k):
    """k * pt for the plain integer k < 2^256, by the C oracle's bit-serial double-and-add."""
    return None if pt is None else from_raw96(C.scalar_mul(E.raw96(pt), k.to_bytes(32, "little")))


def decode(enc):
    """(status, point): O.g1_decompress, unchecked; a refused encoding gives BAD_POINT."""
    try:
        return 0, O.g1_decompress(enc, False)
    except ValueError:
        return BAD_POINT, None


class Case:
    """name; trackers [(r_G 48 bytes, k_r_G 48 bytes)]; ks [integers below 2^256]; tile (the native call's tile_bases, 0 = default);
    then, from the oracle: tracker_status, k_status, bits {(i, j)}, bitmap (bytes: T x ceil(V / 64) little-endian 64-bit words)."""

    def __init__(self, name, trackers, ks, tile=0):
        self.name, self.trackers, self.ks, self.tile = name, [(bytes(r), bytes(s)) for r, s in trackers], list(ks), tile
        T, V = len(self.trackers), len(self.ks)
        self.words = (V + 63) // 64
        dec = [(decode(r), decode(s)) for r, s in self.trackers]
        self.tracker_status = [BAD_POINT if a[0] or b[0] else 0 for a, b in dec]
        self.k_status = [BAD_SCALAR if k >= R else 0 for k in self.ks]
        self.bits = set()
        for i, ((_, rp), (_, sp)) in enumerate(dec):
            if self.tracker_status[i]:
                continue
            for j, k in enumerate(self.ks):
                if not self.k_status[j] and omul(rp, k) == sp:
                    self.bits.add((i, j))
        rows = [[0] * self.words for _ in range(T)]
        for i, j in self.bits:
            rows[i][j >> 6] |= 1 << (j & 63)
        self.bitmap = b"".join(w.to_bytes(8, "little") for row in rows for w in row)

    @property
    def trackers96(self):
        return b"".join(r + s for r, s in self.trackers)

    @property
    def ks32(self):
        return b"".join(k.to_bytes(32, "little") for k in self.ks)


def _tracker(rp, sp):
    return O.g1_compress(rp), O.g1_compress(sp)


def _planted(name, rng, T, V, plant, tile=0):
    """T trackers of G1 x V distinct secrets; plant = {tracker: [columns]}: the columns of one tracker all hold the SAME secret (the
    only way one tracker has two openers), everything else must come out zero."""
    ks = [rng.randrange(2, R) for _ in range(V)]
    assert len(set(ks)) == V
    for cols in plant.values():
        for j in cols[1:]:
            ks[j] = ks[cols[0]]
    trackers = []
    for i in range(T):
        rp = O.g1_mul(O.G1_GEN, rng.randrange(1, R))
        k = ks[plant[i][0]] if i in plant else rng.randrange(2, R)
        trackers.append(_tracker(rp, omul(rp, k)))
    c = Case(name, trackers, ks, tile)
    want = {(i, j) for i, cols in plant.items() for j in cols}
    # a planted column's secret may be shared with another tracker's planted columns only where the plan says so
    assert c.bits == {(i, j) for i in plant for j in range(V) if ks[j] == ks[plant[i][0]]} and want <= c.bits, name
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case}.  Fails while building if the small-order cases do not drive the windowed sum into every event of EVENTS."""
    rng = random.Random(0x7AC4E5)
    out = {}

    def put(c):
        assert c.name not in out
        out[c.name] = c

    # ---- the layout: the smallest shapes at which a word, a lane or a tile edge can go wrong
    put(_planted("1 x 1", rng, 1, 1, {0: [0]}))
    put(_planted("3 x 65", rng, 3, 65, {0: [0], 1: [63], 2: [64]}))                         # second word: one live lane
    put(_planted("5 x 64, tile 2", rng, 5, 64, {0: [0], 1: [63], 2: [1, 62], 3: [2], 4: [33]}, tile=2))      # tiles {0,1} {2,3} {4}: first and last of each
    put(_planted("2 x 130", rng, 2, 130, {0: [0, 63, 64, 127], 1: [128, 129]}))
    assert all(len(out[n].bits) == m for n, m in (("1 x 1", 1), ("3 x 65", 3), ("5 x 64, tile 2", 6), ("2 x 130", 6)))

    # ---- near misses
    g = [O.g1_mul(O.G1_GEN, rng.randrange(1, R)) for _ in range(3)]
    k = rng.randrange(2, R - 1)
    kg = omul(g[0], k)
    put(Case("near misses", [_tracker(g[0], kg), _tracker(g[0], O.g1_neg(kg)), _tracker(g[0], omul(g[0], k + 1)), _tracker(g[0], omul(g[1], k)),
                             _tracker(kg, g[0])], [k]))
    assert out["near misses"].bits == {(0, 0)}
    assert O.g1_compress(kg)[1:] == O.g1_compress(O.g1_neg(kg))[1:]                         # the same x, the other sign bit

    # ---- scalars and identities
    ks = [0, 1, R - 1, R, (1 << 256) - 1, k]
    trk = [_tracker(g[0], None), _tracker(g[0], g[0]), _tracker(g[0], O.g1_neg(g[0])), _tracker(None, None), _tracker(None, g[0]), _tracker(g[0], kg)]
    c = Case("scalars and identities", trk, ks)
    assert c.k_status == [0, 0, 0, BAD_SCALAR, BAD_SCALAR, 0]
    assert c.bits == {(0, 0), (1, 1), (2, 2), (5, 5)} | {(3, j) for j in (0, 1, 2, 5)}       # the dense row: every live secret
    put(c)

    # ---- the whole curve: bases of order 3, 11, 33 and torsion + G1 under integers below r
    m = M.cases()
    bases = {label: (pt, order) for label, pt, order in m.bases}
    small = [("t3", 3), ("-t3", 3), ("order 11", 11), ("t3 + order 11", 33)]
    ks = [s for s in m.scalars if s < R][:24] + [rng.randrange(R) for _ in range(12)]
    count = {}
    for label, order in small:
        assert bases[label][1] == order
        for s in ks:
            ev, end = window_events(order, s)
            assert end == s % order
            for e in ev:
                count[e] = count.get(e, 0) + 1
    missing = [e for e in EVENTS if not count.get(e)]
    assert not missing, f"no (base, secret) pair drives the windowed sum into: {missing}"
    trk = []
    for label in [l for l, _ in small] + ["t3 + g1", "order 11 + g1", "g1 a"]:
        pt, order = bases[label]
        trk += [_tracker(pt, omul(pt, ks[5])), _tracker(pt, omul(pt, ks[-1])), _tracker(pt, None), _tracker(pt, pt)]
    c = Case("whole curve", trk, ks)
    for i in range(len(small) * 4):                        # a base of small order: every secret in the residue class opens it
        pt, order = bases[small[i // 4][0]]
        _, sp = decode(c.trackers[i][1])
        assert {j for (ii, j) in c.bits if ii == i} == {j for j, s in enumerate(ks) if E.mul_any(pt, s % order) == sp}
    assert any(len([1 for (ii, _) in c.bits if ii == i]) > 4 for i in range(4))
    c.events = count
    put(c)

    # ---- bad encodings in r_G and in k_r_G, good neighbours
    e = E.cases()
    bad = {}
    for label, enc in e.encodings:
        if E.expect_decode(enc, False)[0] != E.OK:
            bad.setdefault(label, enc)
    assert {"x>=p", "x<p non-square", "flag clear"} <= set(bad)
    k2 = rng.randrange(2, R)
    good = _tracker(g[1], omul(g[1], k2))
    trk = [good]
    for label in ("x>=p", "x<p non-square", "flag clear", "x=p"):
        trk += [(bad[label], good[1]), good, (good[0], bad[label]), good]
    c = Case("bad encodings", trk, [k2, k])
    assert c.tracker_status == [0] + [BAD_POINT, 0, BAD_POINT, 0] * 4 and c.bits == {(i, 0) for i in range(0, len(trk), 2)}
    put(c)

    # ---- data made by the reference: every tracker of the opening prover's vectors against every secret of them
    with open(os.path.join(ROOT, "tests", "golden", "opening_prover_vectors.json")) as f:
        gold = json.load(f)
    items = [(x["name"], x) for x in gold["cases"] if not x.get("raises")] + [(f"sequence {i}", x) for i, x in enumerate(gold["sequence"]["items"])]
    c = Case("reference vectors", [(bytes.fromhex(x["r_G"]), bytes.fromhex(x["k_r_G"])) for _, x in items],
             [int.from_bytes(bytes.fromhex(x["k"]), "little") for _, x in items])
    assert not any(c.tracker_status[:12]) and 0 < sum(1 for t in c.tracker_status if t) < 4       # (the recorded sequence holds items the reference refuses)
    for i, (name, _) in enumerate(items):
        assert ((i, i) in c.bits) == (name != "k_r_G != k r_G" and not c.tracker_status[i] and not c.k_status[i]), name
    put(c)

    # ---- seeded differential: 16 x 130, about ten planted matches
    plant = {}
    for _ in range(10):
        plant.setdefault(rng.randrange(16), []).append(rng.randrange(130))
    put(_planted("differential 16 x 130", rng, 16, 130, plant, tile=0))
    return out
