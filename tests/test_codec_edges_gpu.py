"""The device's wire codec and its three subgroup tests at the adversarial encodings of tests/codec_edge_cases.py.  Needs an MI355X.

What is pinned, every expected value being the oracle's (never another path of the product):
  a. k_batch_decompress<true,2>, <false,3> and <false,2>: status class and 96 output bytes per lane for a y next to (p-1)/2 and an x next to
     p at every 32-bit word, the flag patterns, with refused lanes at block edges;
  b. k_batch_decompress_row (cg1_batch_decompress_rows): every valid edge encoding against the oracle, every refused one at the first, a
     middle and the last position;
  c. the compress rule in k_batch_compress and in k_fixed_finish / compress_words (through a light table whose bases are the edge points);
  d. k_subgroup_row (cg1_batch_subgroup on the device) and
  e. k_subgroup_flags (cg1_subgroup_flags_enqueue) on points of order 3, 11, 10177, 859267, 52437899, their sums with points of G1,
     points of full order and their pure parts: the double-and-add of [|z|]P runs into P + P, P - P and the identity on these.
Out of scope: the verifier front-end's compress48 and the generator kernel's output only ever see points the device computed itself,
which no caller can steer next to (p-1)/2."""
import ctypes
import math

import pytest

import codec_edge_cases as E
from oracle import bls12_381 as O

pytestmark = pytest.mark.gpu
NEG = 1 << 31


@pytest.fixture(scope="module")
def c():
    return E.cases()


@pytest.fixture(scope="module")
def ctx(native_lib):
    cx = native_lib.Context(0)
    yield cx
    cx.close()


def status(N, cls):
    return {E.OK: N.OK, E.ENCODING: N.ERR_ENCODING, E.NOT_ON_CURVE: N.ERR_NOT_ON_CURVE, E.NOT_IN_SUBGROUP: N.ERR_NOT_IN_SUBGROUP}[cls]


def lane_decode(N, ctx, encs, check):
    """cg1_batch_decompress_device over buffers pre-filled with 0xEE -> ([affine96], [status byte])."""
    n = len(encs)
    d_in, d_out, d_st = ctx.alloc(48 * n), ctx.alloc(96 * n + 96), ctx.alloc(n + 16)
    try:
        d_in.upload(b"".join(encs))
        d_out.upload(b"\xee" * (96 * n + 96))
        d_st.upload(b"\xee" * (n + 16))
        ctx.check(N.cg1_batch_decompress_device(ctx.handle, d_in.ptr, d_out.ptr, d_st.ptr, n, check))
        out, st = d_out.download(), d_st.download()
    finally:
        d_in.free(); d_out.free(); d_st.free()
    assert out[96 * n:] == b"\xee" * 96 and st[n:] == b"\xee" * 16             # nothing written past lane n - 1
    return [out[96 * i: 96 * i + 96] for i in range(n)], list(st[:n])


def assert_lanes(N, encs, got, st, check, tag):
    for i, e in enumerate(encs):
        cls, raw = E.expect_decode(e, bool(check))
        assert st[i] == status(N, cls) and got[i] == raw, (tag, i, e.hex(), cls, st[i])


# ------------------------------------------------------------------ a. the lane decoder
@pytest.mark.parametrize("check,waves", [(1, 3), (0, 3), (0, 2)], ids=["checked", "unchecked_w3", "unchecked_w2"])
def test_lane_decoder_at_every_edge(native_lib, ctx, c, check, waves):
    """Every edge encoding between valid G1 encodings; n = 1, 127, 128, 129 and the whole list, rotated so that a refused encoding (one of
    each class refused without the subgroup test) sits in lane 0, 127 (the last of block 0), 128 (alone in block 1) and in the last lane.
    A refused lane leaves zeros, and its neighbours what the oracle decodes."""
    N = native_lib
    base = []
    for f, (_, e) in zip(c.fillers, c.encodings):
        base += [O.g1_compress(f), e]
    L = len(base)
    assert L == 2 * len(c.encodings) >= 130
    pick = {}
    for i, e in enumerate(base):
        cls = E.expect_decode(e, False)[0]
        label = c.encodings[i // 2][0] if i & 1 else "g1"
        if cls != E.OK:
            pick.setdefault(label, i)
    b = [pick["x>=p"], pick["x<p non-square"], pick["flag clear"], pick["x=p"]]

    def rot(at, src):
        s = (src - at) % L
        r = base[s:] + base[:s]
        assert r[at] == base[src]
        return r

    r0, r127, r128, rlast = rot(0, b[0]), rot(127, b[1]), rot(128, b[2]), rot(L - 1, b[3])
    one_valid = [O.g1_compress(c.boundary[0][2])]
    runs = [("n=1 refused", r0[:1]), ("n=1 boundary", one_valid), ("n=127", r0[:127]), ("n=128", r127[:128]), ("n=129", r128[:129]),
            ("all@0", r0), ("all@127", r127), ("all@128", r128), ("all@last", rlast)]
    ctx.set_param("decompress_waves", waves)
    try:
        for tag, encs in runs:
            got, st = lane_decode(N, ctx, encs, check)
            assert_lanes(N, encs, got, st, check, tag)
    finally:
        ctx.set_param("decompress_waves", 3)
    assert all(E.expect_decode(r[at], False)[0] != E.OK for at, r in ((0, r0), (127, r127), (128, r128), (L - 1, rlast)))
    classes = {E.expect_decode(e, bool(check))[0] for e in base}
    assert classes == {E.OK, E.ENCODING, E.NOT_ON_CURVE} | ({E.NOT_IN_SUBGROUP} if check else set())


def test_lane_decoder_subgroup_verdicts(native_lib, ctx, c):
    """check = 1 on the oracle's encoding of every point of the subgroup list: OK or NOT_IN_SUBGROUP exactly as the oracle's [r]P says."""
    N = native_lib
    pts = [p for _, p in c.subgroup]
    encs = [O.g1_compress(p) for p in pts]
    got, st = lane_decode(N, ctx, encs, 1)
    for (label, p), g, s in zip(c.subgroup, got, st):
        inside = O.g1_in_subgroup(p)
        assert s == (N.OK if inside else N.ERR_NOT_IN_SUBGROUP), (label, s)
        assert g == (E.raw96(p) if inside else bytes(96)), label
    got, st = lane_decode(N, ctx, encs, 0)                                       # and unchecked: every one decodes to itself
    assert st == [N.OK] * len(pts) and got == [E.raw96(p) for p in pts]


# ------------------------------------------------------------------ b. the row decoder
def rows_decode(N, ctx, encs):
    n = len(encs)
    aff, bad = ctypes.create_string_buffer(96 * n), ctypes.c_size_t(1 << 40)
    rc = N.cg1_batch_decompress_rows(ctx.handle, b"".join(encs), n, None, aff, ctypes.byref(bad))
    return rc, bad.value, aff.raw


def test_row_decoder_every_valid_edge(native_lib, ctx, c):
    """Every valid edge encoding (boundary points, x next to p, +-T3, the lenient identities) with n = 0, 1, 2, 3 mod 4 and the tiny
    batches of one partial wave: affine96 against the oracle for EVERY point."""
    N = native_lib
    valid = [e for _, e in c.encodings if E.expect_decode(e, False)[0] == E.OK]
    V = len(valid)
    assert V >= 60 and {lab for lab, e in c.encodings if E.expect_decode(e, False)[0] == E.OK} == {"boundary", "boundary inner", "x<p square", "x=0", "infinity", "infinity+sign", "infinity+junk"}
    sizes = [V, V - 1, V - 2, V - 3, 1, 2, 3]
    assert {n % 4 for n in sizes[:4]} == {0, 1, 2, 3}
    for n in sizes:
        for encs in (valid[:n], valid[V - n:]):                                 # from either end: every encoding is in some batch of each size
            rc, _, aff = rows_decode(N, ctx, encs)
            assert rc == N.OK
            for i, e in enumerate(encs):
                assert aff[96 * i: 96 * i + 96] == E.expect_decode(e, False)[1], (n, i, e.hex())


def test_row_decoder_refusals_by_position(native_lib, ctx, c):
    """Every refused encoding at the first, a middle and the last position of a batch of valid edge encodings (whose size runs through
    the residues mod 4, so the last position is every row of a wave): the status and the first failing index the oracle implies."""
    N = native_lib
    valid = [e for _, e in c.encodings if E.expect_decode(e, False)[0] == E.OK]
    refused = [(lab, e) for lab, e in c.encodings if E.expect_decode(e, False)[0] != E.OK]
    assert {lab for lab, _ in refused} == {"x>=p", "x=p", "x=2^381-1", "flag clear", "x<p non-square", "x=p-1"}
    for t, (lab, e) in enumerate(refused):
        n = len(valid) - t % 4
        want = status(N, E.expect_decode(e, False)[0])
        for pos in (0, n // 2 + t % 3, n - 1):
            encs = valid[:n]
            encs[pos] = e
            rc, bad, _ = rows_decode(N, ctx, encs)
            assert (rc, bad) == (want, pos), (lab, e.hex(), pos, n)
    encs = valid[:40]
    encs[33], encs[6], encs[7] = refused[0][1], refused[-1][1], refused[1][1]     # several: the first one's
    assert rows_decode(N, ctx, encs)[:2] == (status(N, E.expect_decode(refused[-1][1], False)[0]), 6)


# ------------------------------------------------------------------ c. compress
def test_device_compress_at_the_sign_boundary(native_lib, ctx, c):
    """k_batch_compress on all 48 boundary points, the 44 from the near side, the x-range accepts, +-T3 and the identity."""
    N = native_lib
    pts = c.boundary_pts + [p for p in c.valid_points if p not in c.boundary_pts] + [None]
    n = len(pts)
    d_in, d_out = ctx.alloc(96 * n), ctx.alloc(48 * n + 48)
    d_in.upload(b"".join(E.raw96(p) for p in pts))
    d_out.upload(b"\xee" * (48 * n + 48))
    ctx.check(N.cg1_batch_compress_device(ctx.handle, d_in.ptr, d_out.ptr, n))
    got = d_out.download()
    d_in.free(); d_out.free()
    want = [O.g1_compress(p) for p in pts]
    assert set(c.inner_pts) <= set(pts) and sum(1 for w in want if w[0] & 0x20) >= 46 and sum(1 for w in want if not w[0] & 0x60) >= 46
    for i, p in enumerate(pts):
        assert got[48 * i: 48 * i + 48] == want[i], (i, p)
    assert got[48 * n:] == b"\xee" * 48


def test_table_msm_compress_at_the_sign_boundary(native_lib, ctx, c):
    """The second device copy of the rule (compress_words in k_fixed_finish): a light table whose bases are the edge points, one term
    of scalar 1 per MSM, the base and the negated base (bit 31 of the index): 48 bytes each, against the oracle."""
    pts = list(dict.fromkeys(c.boundary_pts + c.valid_points))
    assert set(c.boundary_pts + c.inner_pts) <= set(pts)
    tab = ctx.light_table(b"".join(E.raw96(p) for p in pts), len(pts))
    try:
        idx = list(range(len(pts))) + [i | NEG for i in range(len(pts))]
        got = ctx.light_msm_host(tab, idx, (1).to_bytes(32, "little") * len(idx), list(range(len(idx) + 1)), compressed=True)
    finally:
        tab.free()
    for i, j in enumerate(idx):
        p = pts[j & ~NEG]
        assert got[i] == O.g1_compress(O.g1_neg(p) if j & NEG else p), (i, bool(j & NEG))


# ------------------------------------------------------------------ d. one wave per point
def test_subgroup_rows_on_small_orders(native_lib, ctx, c):
    """cg1_batch_subgroup served by k_subgroup_row (n = 32, 33, 32 and 120): flags[i] = 1 iff the oracle's [r]P is the identity; every point
    of the list is in two of the four calls."""
    N = native_lib
    sub, fill = c.subgroup, [("g1", f) for f in c.fillers]
    assert len(sub) == 66
    batches = [sub[:22] + fill[:10], sub[22:44] + fill[:11], fill[:5] + sub[44:] + fill[5:10], sub + fill[:54]]
    assert [len(b) for b in batches] == [32, 33, 32, 120]
    for batch in batches:
        n = len(batch)
        flags, on_dev = ctypes.create_string_buffer(b"\xee" * (n + 8), n + 8), ctypes.c_int(-1)
        ctx.check(N.cg1_batch_subgroup(ctx.handle, b"".join(E.raw96(p) for _, p in batch), n, flags, ctypes.byref(on_dev)))
        assert on_dev.value == 1
        for i, (label, p) in enumerate(batch):
            assert flags.raw[i] == (1 if E.in_g1(p) else 0), (n, i, label)
        assert flags.raw[n:] == b"\xee" * 8
    assert ("identity", None) in batches[0] and E.in_g1(None)


# ------------------------------------------------------------------ e. one quad per selected point
@pytest.mark.parametrize("n_proofs,stride,offsets", [(70, 3, [1]), (7, 12, [11, 0, 5, 2, 9, 3, 7, 4, 10, 6]), (5, 20, [19, 0, 17, 2, 15, 4, 13, 6, 11, 8, 9, 10, 7, 12, 5, 14])],
                         ids=["k1", "k10", "k16"])
def test_subgroup_flags_on_small_orders(native_lib, ctx, c, n_proofs, stride, offsets):
    """cg1_subgroup_flags_enqueue + cg1_side_sync over an n_proofs x stride array: every point of the subgroup list under a selected
    offset (the rest of the selected slots hold points of G1, every slot NOT selected holds the order-3 point), k = 1, 10, 16; 280 lanes
    in the first two shapes, so the last block is partial.  flags = 1 iff the oracle says the point is NOT in G1; the identity gives 0;
    exactly n_proofs * k bytes are written."""
    N = native_lib
    k = len(offsets)
    slots = n_proofs * k
    sub = c.subgroup
    assert slots >= len(sub) and len(set(offsets)) == k and max(offsets) < stride and (k == 16 or (slots * 4) % 64 != 0)
    # selected slot s = proof * k + j holds sub[(3 s) % slots] when that index exists (3 is coprime to the slot counts), else a point of G1
    assert math.gcd(3, slots) == 1
    cell = [[E.T3] * stride for _ in range(n_proofs)]
    want = []
    for s in range(slots):
        t = (3 * s) % slots
        label, p = sub[t] if t < len(sub) else ("g1", c.fillers[t % len(c.fillers)])
        cell[s // k][offsets[s % k]] = p
        want.append((label, 0 if E.in_g1(p) else 1))
    assert [w for lab, w in want if lab == "identity"] == [0]
    placed = [p for row in cell for j, p in enumerate(row) if j in offsets]
    assert all(p in placed for _, p in sub)
    raw = b"".join(E.raw96(p) for row in cell for p in row)
    d_aff, d_fl = ctx.alloc(len(raw)), ctx.alloc(slots + 64)
    try:
        d_aff.upload(raw)
        d_fl.upload(b"\xee" * (slots + 64))
        offs = (ctypes.c_uint32 * k)(*offsets)
        ctx.check(N.cg1_subgroup_flags_enqueue(ctx.handle, d_aff.ptr, stride, n_proofs, offs, k, d_fl.ptr))
        ctx.check(N.cg1_side_sync(ctx.handle))
        got = d_fl.download()
    finally:
        d_aff.free(); d_fl.free()
    for s, (label, w) in enumerate(want):
        assert got[s] == w, (s, label, got[s])
    assert got[slots:] == b"\xee" * 64
    assert 0 < sum(w for _, w in want) < slots
