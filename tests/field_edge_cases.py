"""Operands and plain-int references shared by tests/test_field_edges.py (host) and tests/test_field_edges_gpu.py (device): the Fr edge
list, Python replays of fr_inv_binary's loop and of the device's 32-bit-limb product (to PROVE that a chosen input reaches a chosen
branch), and the packing of the 64-byte items cg1_probe_fr_ops / cg1_fr_ops_host take."""
import ctypes
import random

R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
MONT = 1 << 256
MONT_INV = pow(MONT, -1, R_MOD)
R1, R2 = MONT % R_MOD, MONT * MONT % R_MOD

OP_MUL, OP_ADD, OP_SUB, OP_NEG, OP_FROM_LE32, OP_FROM_LE64_WIDE, OP_TO_LE32, OP_INV, OP_INV_BINARY, OP_POW_U64 = range(10)


def fr_edges(n_random=200, seed=0xF2):
    """The edge list (every entry below r, so each is both a value and a canonical Montgomery word), then seeded random values."""
    r = R_MOD
    e = [0, 1, 2, 3, 4, r - 1, r - 2, (r + 1) // 2, (r - 1) // 2, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 1 << 64, 1 << 128, 1 << 254,
         (1 << 254) - 1, R1, R2, r - (1 << 32)]
    e += [0xFFFFFFFF << (32 * i) for i in range(7)]                      # one 32-bit half all ones ...
    e += [((r >> 224) - 1) << 224 | ((1 << 224) - 1)]                    # ... and the top half as far as r allows, all ones below it
    assert all(0 <= v < r for v in e)
    rng = random.Random(seed)
    return e + [rng.randrange(r) for _ in range(n_random)]


# first operands of fr_mul that are NOT canonical (fr_from_le64_wide feeds it raw 256-bit halves)
NONCANONICAL = [(1 << 256) - 1, R_MOD, R_MOD + 1, 2 * R_MOD, 2 * R_MOD + 1, (1 << 255), (1 << 256) - (1 << 32), ((1 << 256) - 1) ^ (0xFFFFFFFF << 96),
                (1 << 256) - R_MOD]


def inv_binary_k(a):
    """The number of steps fr_inv_binary's loop takes on the Montgomery word a (its `k`): the same four-way step, in ints."""
    u, w, k = R_MOD, a, 0
    while w:
        if u % 2 == 0:
            u //= 2
        elif w % 2 == 0:
            w //= 2
        elif u > w:
            u = (u - w) // 2
        else:
            w = (w - u) // 2
        k += 1
    return k


def device_mul_t9(a, b):
    """Replay of the device's fr_mul (CIOS over eight 32-bit limbs): (result, whether the ninth word `t9` was ever non-zero)."""
    M32 = 0xFFFFFFFF
    A, B, M = ([(v >> (32 * i)) & M32 for i in range(8)] for v in (a, b, R_MOD))
    ninv = (-pow(R_MOD, -1, 1 << 32)) % (1 << 32)
    t, seen = [0] * 9, False
    for i in range(8):
        c = 0
        for j in range(8):
            p = A[j] * B[i] + t[j] + c
            t[j], c = p & M32, p >> 32
        s = t[8] + c
        t[8], t9 = s & M32, s >> 32
        seen = seen or t9 != 0
        m = (t[0] * ninv) & M32
        c = (m * M[0] + t[0]) >> 32
        for j in range(1, 8):
            p = m * M[j] + t[j] + c
            t[j - 1], c = p & M32, p >> 32
        s2 = t[8] + c
        t[7], t[8] = s2 & M32, t9 + (s2 >> 32)
    v = sum(x << (32 * i) for i, x in enumerate(t[:8]))
    if t[8] or v >= R_MOD:
        v = (v - R_MOD) % (1 << 256)
    return v, seen


def items(pairs):
    """64-byte items: a at byte 0, b at byte 32 (little-endian)."""
    return b"".join(a.to_bytes(32, "little") + b.to_bytes(32, "little") for a, b in pairs)


def run(fn, op, raw):
    """fn(op, in, n, out) over 64-byte items -> [(result as int, flag word)]."""
    n = len(raw) // 64
    out = ctypes.create_string_buffer(64 * n)
    rc = fn(op, raw, n, out)
    assert rc == 0, rc
    o = out.raw
    assert all(o[64 * i + 40: 64 * i + 64] == bytes(24) for i in range(n))
    return [(int.from_bytes(o[64 * i: 64 * i + 32], "little"), int.from_bytes(o[64 * i + 32: 64 * i + 40], "little")) for i in range(n)]


def fr_cases():
    """{op: (items, expected [(result, flag)])} over the edge list: every operation, expected values from Python ints alone."""
    r, E = R_MOD, fr_edges()
    rng = random.Random(0xF3)
    head = E[:27]
    pairs = [(a, b) for a in head for b in head] + [(a, rng.choice(E)) for a in E] + [(rng.choice(E), b) for b in E]
    wide = [(a, b) for a in NONCANONICAL for b in head + E[27:40]]
    assert any(device_mul_t9(a, b)[1] for a, b in wide), "no non-canonical product reaches the ninth word"
    c = {}
    mp = pairs + wide
    c[OP_MUL] = (mp, [(a * b * MONT_INV % r, 1) for a, b in mp])
    c[OP_ADD] = (pairs, [((a + b) % r, 1) for a, b in pairs])
    c[OP_SUB] = (pairs, [((a - b) % r, 1) for a, b in pairs])
    c[OP_NEG] = ([(a, 0) for a in E], [((-a) % r, 1) for a in E])
    le = E + [r, r + 1, (1 << 256) - 1, 2 * r, 1 << 255]
    c[OP_FROM_LE32] = ([(v, 0) for v in le], [(v * MONT % r, 1) if v < r else (0, 0) for v in le])
    w = [(0, 0), ((1 << 256) - 1, (1 << 256) - 1), (0, r), (r - 1, r - 1), (r, r), ((1 << 256) - 1, 0), (0, (1 << 256) - 1)]
    w += [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(200)] + [(a, rng.choice(E)) for a in head]
    c[OP_FROM_LE64_WIDE] = (w, [((lo + (hi << 256)) % r * MONT % r, 1) for lo, hi in w])
    c[OP_TO_LE32] = ([(a, 0) for a in E], [(a * MONT_INV % r, 1) for a in E])
    inv = [(pow(a, -1, r) * R2 % r if a else 0, 1) for a in E]             # A = a R  ->  a^-1 R = A^-1 R^2
    c[OP_INV] = ([(a, 0) for a in E], inv)
    c[OP_INV_BINARY] = ([(a, 0) for a in E], inv)
    pw = [(a, e) for a in head for e in (0, 1, 2, 1 << 63, (1 << 64) - 1)] + [(a, rng.getrandbits(64)) for a in E[27:60]]
    c[OP_POW_U64] = (pw, [(pow(a * MONT_INV, e, r) * MONT % r, 1) for a, e in pw])
    return c


def inv_binary_step_counts():
    """k of every inversion input of fr_cases: the test asserts the branches these reach."""
    return [inv_binary_k(a) for a in fr_edges() if a]
