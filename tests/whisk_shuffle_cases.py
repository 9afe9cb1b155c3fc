"""Inputs and expected outputs for the front of the batched Whisk shuffle prover, shared by tests/test_whisk_shuffle_prover.py (the host
twin cg1_whisk_shuffle_front_emulate) and tests/test_whisk_shuffle_prover_gpu.py (cg1_whisk_shuffle_front on the device): the fixture
cases of tests/golden/shuffle_device_vectors.json that store their points, edge inputs at ell = 4 and the refusals.  Every expected value
is computed by oracle/bls12_381.py (g1_decompress, g1_mul, g1_compress, compute_MSM) -- no product code -- once per process."""
import functools
import json
import os

from oracle import bls12_381 as O

from codec_edge_cases import enc_x, raw96, x_range_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, P = O.R, O.P
NB = 4
INF = b"\xc0" + bytes(47)
HALVES = ("r_G", "k_r_G")


def golden(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name)))["cases"]


def mul(pt, k):
    return None if pt is None or k % R == 0 else O.g1_mul(pt, k)


class Front:
    """One prover's inputs as bytes and ints, and what the front must give back for them."""

    def __init__(self, name, crs, trackers, perm, k, mbl):
        self.name, self.crs, self.ell = name, crs, len(trackers)
        self.trackers, self.perm, self.k, self.mbl = [(bytes(r), bytes(s)) for r, s in trackers], list(perm), k, list(mbl)

    trackers96 = property(lambda s: b"".join(r + kr for r, kr in s.trackers))
    k32 = property(lambda s: s.k.to_bytes(32, "little"))
    mbl32 = property(lambda s: b"".join(b.to_bytes(32, "little") for b in s.mbl))

    @functools.cached_property
    def expected(self):
        """-> dict(rs, tu, post, row, m48) of bytes, by the oracle."""
        ell = self.ell
        vR = [O.g1_decompress(r) for r, _ in self.trackers]
        vS = [O.g1_decompress(s) for _, s in self.trackers]
        vT, vU = [mul(vR[j], self.k) for j in self.perm], [mul(vS[j], self.k) for j in self.perm]
        row = list(self.perm) + self.mbl
        M = O.compute_MSM(self.crs, row)
        return {"rs": b"".join(raw96(p) for p in vR + vS), "tu": b"".join(raw96(p) for p in vT + vU),
                "post": b"".join(O.g1_compress(vT[i]) + O.g1_compress(vU[i]) for i in range(ell)),
                "row": b"".join(v.to_bytes(32, "little") for v in row), "m48": O.g1_compress(M)}


@functools.lru_cache(maxsize=None)
def fixture_fronts():
    """The three cases of shuffle_device_vectors.json that store their points (ell = 4, 12, 28), with their vec_R / vec_S encodings as
    trackers: -> [(Front, case)]; the case's vec_T, vec_U and M are what the front must reproduce."""
    out = []
    for c in golden("shuffle_device_vectors.json"):
        if "vec_G" not in c:
            continue
        crs = tuple(O.g1_decompress(bytes.fromhex(h)) for h in c["vec_G"] + c["vec_H"])
        f = Front(f"fixture ell = {c['ell']}", crs, [(bytes.fromhex(r), bytes.fromhex(s)) for r, s in zip(c["vec_R"], c["vec_S"])], c["permutation"],
                  int.from_bytes(bytes.fromhex(c["k"]), "little"), [int.from_bytes(bytes.fromhex(h), "little") for h in c["vec_m_blinders"]])
        out.append((f, c))
    assert [f.ell for f, _ in out] == [4, 12, 28]
    return out


def crs_encodings(ell=4):
    """vec_G | vec_H encodings of the fixture case of that ell."""
    c = next(c for c in golden("shuffle_device_vectors.json") if c["ell"] == ell)
    return [bytes.fromhex(h) for h in c["vec_G"] + c["vec_H"]]


def sign_bit(enc):
    return bool(enc[0] & 0x20)


@functools.lru_cache(maxsize=None)
def edge_fronts():
    """{name: Front} at ell = 4 over the first fixture case's CRS."""
    base, _ = fixture_fronts()[0]
    crs = base.crs
    g = lambda k: O.g1_compress(O.g1_mul(O.G1_GEN, k))
    # trackers with both values of the sign bit among the inputs (asserted by the tests on inputs and outputs)
    pts = [g(k) for k in range(0x51, 0x71)]
    lo = [e for e in pts if not sign_bit(e)][:4]
    hi = [e for e in pts if sign_bit(e)][:4]
    assert len(lo) == 4 and len(hi) == 4
    mixed = [(lo[0], hi[0]), (hi[1], lo[1]), (lo[2], lo[3]), (hi[2], hi[3])]
    vx = x_range_cases()[1][3][1]                                      # a valid x, as junk under the infinity flag
    lenient = [enc_x(vx, 0xC0), enc_x(0, 0xE0), enc_x((1 << 381) - 1, 0xC0), enc_x(1, 0xC0)]
    mbl = [0x1111, R - 1, 0, 7]
    perm = [2, 0, 3, 1]
    k = 0x5EED5EED5EED5EED5EED5EED5EED5EED5EED5EED5EED5EED5EED % R
    fronts = [
        Front("canonical identity", crs, [(INF, mixed[0][1]), mixed[1], (mixed[2][0], INF), (INF, INF)], perm, k, mbl),
        Front("lenient identities", crs, [(lenient[0], mixed[0][1]), (lenient[1], lenient[2]), mixed[2], (mixed[3][0], lenient[3])], perm, k, mbl),
        Front("k = 0", crs, mixed, perm, 0, mbl),
        Front("k = 1", crs, mixed, perm, 1, mbl),
        Front("k = r - 1", crs, mixed, perm, R - 1, mbl),
        Front("no bijection", crs, mixed, [1, 1, 3, 1], k, mbl),
        Front("repeated trackers", crs, [mixed[0], mixed[0], mixed[1], mixed[0]], perm, k + 1, mbl),
        Front("both signs", crs, mixed, [3, 2, 1, 0], k + 2, [1, 2, 3, 4]),
    ]
    return {f.name: f for f in fronts}


def torsion_encoding():
    """T3 + P for the order-3 point T3 of tests/golden/torsion_vectors.json: on the curve, outside G1."""
    tors = json.load(open(os.path.join(ROOT, "tests", "golden", "torsion_vectors.json")))
    T3 = O.g1_decompress(bytes.fromhex(tors["t3"]))
    pt = O.g1_add(T3, O.g1_mul(O.G1_GEN, 0x5EED))
    assert O.g1_is_on_curve(pt) and not O.g1_in_subgroup(pt)
    return O.g1_compress(pt)


@functools.lru_cache(maxsize=None)
def refusals():
    """[(name, status name, edit, text fragments)]: edit(front) -> a changed copy of a valid ell = 4 front (or a dict of raw overrides for
    the call); the text fragments name the index and the half (the prover is the caller's to check)."""
    non_square = x_range_cases()[2][3][1]
    valid_x = x_range_cases()[1][3][1]

    def tracker(i, half, enc):
        def edit(f):
            t = [list(x) for x in f.trackers]
            t[i][half] = enc
            return Front(f.name, f.crs, t, f.perm, f.k, f.mbl)
        return edit, (f"tracker {i}", HALVES[half])

    def field(**kw):
        def edit(f):
            g = Front(f.name, f.crs, f.trackers, kw.get("perm", f.perm), f.k, f.mbl)
            g.raw = {key: v for key, v in kw.items() if key != "perm"}
            return g
        return edit, ()

    big = (1 << 256) - 1
    s32 = lambda v: v.to_bytes(32, "little")
    out = [
        ("no compression flag", "ERR_ENCODING", *tracker(1, 0, enc_x(valid_x, 0x00))),
        ("x = p", "ERR_ENCODING", *tracker(2, 1, enc_x(P, 0x80))),
        ("x = 2^381 - 1", "ERR_ENCODING", *tracker(0, 1, enc_x((1 << 381) - 1, 0xA0))),
        ("x with no point", "ERR_NOT_ON_CURVE", *tracker(3, 0, enc_x(non_square, 0x80))),
        ("outside G1", "ERR_NOT_IN_SUBGROUP", *tracker(2, 0, torsion_encoding())),
        ("outside G1, second half", "ERR_NOT_IN_SUBGROUP", *tracker(3, 1, torsion_encoding())),
        ("k = r", "ERR_ENCODING", *field(k32=s32(R))),
        ("k = 2^256 - 1", "ERR_ENCODING", *field(k32=s32(big))),
        ("a blinder = r", "ERR_ENCODING", *field(mbl32=s32(5) + s32(6) + s32(R) + s32(7))),
        ("a blinder = 2^256 - 1", "ERR_ENCODING", *field(mbl32=s32(5) + s32(6) + s32(7) + s32(big))),
        ("perm entry = ell", "ERR_ARG", *field(perm=[0, 1, 4, 2])),
    ]
    return out
