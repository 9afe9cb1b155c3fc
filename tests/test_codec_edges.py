"""The host's wire codec and subgroup test (csrc/host_g1.cpp, csrc/lazy_host.cpp) at the adversarial encodings of
tests/codec_edge_cases.py: a y next to (p-1)/2 and an x next to p at every 32-bit word (so both halves of each of the host's 64-bit
words decide some case), the flag patterns, and points of every small order the cofactor has.  Every expected value is the oracle's.
No GPU: these are the host twins of what tests/test_codec_edges_gpu.py asks of the device, and the first check of the fixture itself."""
import ctypes

import pytest

import codec_edge_cases as E
from oracle import bls12_381 as O


@pytest.fixture(scope="module")
def c():
    return E.cases()


def status(N, cls):
    return {E.OK: N.OK, E.ENCODING: N.ERR_ENCODING, E.NOT_ON_CURVE: N.ERR_NOT_ON_CURVE, E.NOT_IN_SUBGROUP: N.ERR_NOT_IN_SUBGROUP}[cls]


def blob_of(N, pt):
    out = ctypes.create_string_buffer(N.POINT_BYTES)
    assert N.cg1_from_affine96(out, E.raw96(pt), 1) == N.OK
    return out.raw


def affine_of(N, blob):
    out = ctypes.create_string_buffer(96)
    N.cg1_to_affine96(out, blob)
    return out.raw


def test_the_fixture_is_what_it_says(c):
    """24 word/side pairs whose deciding word is the pair's own, x-range cases at every word on both sides of p, every refusal class
    present, and expected values that are the oracle's own answers."""
    assert sorted((j, s) for j, s, _ in c.boundary) == sorted((j, s) for j in range(12) for s in ("above", "below"))
    hw = E.words(E.H)
    for j, side, (x, y) in c.boundary:
        yw = E.words(y)
        assert (y * y - x * x * x - 4) % O.P == 0 and yw[j + 1:] == hw[j + 1:] and (yw[j] > hw[j]) == (side == "above") and yw[j] != hw[j]
        assert abs(y - E.H) < (1 << (32 * j)) + E.MAX_STEPS + 2
        for pt in ((x, y), O.g1_neg((x, y))):
            assert pt in c.boundary_pts and not O.g1_in_subgroup(pt)
            assert O.g1_decompress(O.g1_compress(pt)) == pt
    assert E.boundary_points()[0][2][1] == E.H + 5 and E.boundary_points()[1][2][1] == E.H - 4
    assert sorted((j, s) for j, s, _ in c.inner) == sorted((j, s) for j in range(1, 12) for s in ("above", "below"))
    for j, side, (x, y) in c.inner:                                      # word j still decides, by one, against the words below it
        yw, low = E.words(y), (1 << (32 * j)) - 1
        assert yw[j + 1:] == hw[j + 1:] and yw[j] - hw[j] == (1 if side == "above" else -1) and ((y & low) < (E.H & low)) == (side == "above")
        assert (y * y - x * x * x - 4) % O.P == 0 and not O.g1_in_subgroup((x, y)) and {(x, y), O.g1_neg((x, y))} <= set(c.inner_pts)
    assert [j for j, _ in c.x_over_inner] == [j for j, _ in c.x_square_inner] == list(range(1, 12))
    assert [j for j, _ in c.x_over] == [j for j, _ in c.x_square] == [j for j, _ in c.x_non_square] == list(range(12))
    got = {}
    for label, e in c.encodings:
        cls, raw = E.expect_decode(e, False)
        got.setdefault(cls, set()).add(label)
        try:                                                             # the oracle itself, not the builder's reading of it
            pt = O.g1_decompress(e)
            assert cls == E.OK and raw == E.raw96(pt)
        except ValueError:
            assert cls != E.OK and raw == bytes(96)
        if cls == E.OK:
            with_check = E.expect_decode(e, True)
            try:
                assert with_check == (E.OK, E.raw96(O.g1_decompress(e, True)))
            except ValueError:
                assert with_check == (E.NOT_IN_SUBGROUP, bytes(96))
    assert got[E.ENCODING] == {"x>=p", "x=p", "x=2^381-1", "flag clear"} and got[E.NOT_ON_CURVE] == {"x<p non-square", "x=p-1"}
    assert got[E.OK] == {"boundary", "boundary inner", "x<p square", "x=0", "infinity", "infinity+sign", "infinity+junk"}
    for b in (1, 2, 3, 5, O.P - 1, O.P - 2, 1 << 380, E.H):                # the cube root on cubes of every class of a^t (it asserts r^3 == a)
        x = pow(b, 3, O.P)
        assert E.is_cube(x) and pow(E.cube_root(x), 3, O.P) == x
    assert not E.is_cube(2) and {pow(pow(b, 3, O.P), (O.P - 1) // 9, O.P) != 1 for b in (2, 3, 5)} == {True}
    assert [E.in_g1(p) for _, p in c.subgroup] == [O.g1_in_subgroup(p) for _, p in c.subgroup]
    for ell, (a, b) in c.small.items():
        assert a is not None and b is not None and E.mul_any(a, ell) is None and E.mul_any(b, ell) is None
    assert all(E.mul_any(c.small[11][0], k) != c.small[11][1] for k in range(11))


@pytest.mark.parametrize("check", [0, 1])
def test_host_decompress_at_every_edge(native_lib, c, check):
    """cg1_decompress, unchecked and checked: status and point for every encoding, and for the oracle's encoding of every point of the
    subgroup list."""
    N = native_lib
    encs = [e for _, e in c.encodings] + [O.g1_compress(p) for _, p in c.subgroup]
    seen = set()
    for e in encs:
        cls, raw = E.expect_decode(e, bool(check))
        seen.add(cls)
        out = ctypes.create_string_buffer(N.POINT_BYTES)
        rc = N.cg1_decompress(out, e, check)
        assert rc == status(N, cls), (e.hex(), cls)
        if rc == N.OK:
            assert affine_of(N, out.raw) == raw, e.hex()
    assert seen == {E.OK, E.ENCODING, E.NOT_ON_CURVE} | ({E.NOT_IN_SUBGROUP} if check else set())


def test_host_pool_decoder_reports_the_first_bad_index(native_lib, c):
    """cg1_batch_decompress_pool over every valid edge encoding (every point against the oracle), then with each refused encoding at the
    first, a middle and the last position, and two of them at once: the FIRST one's index and status."""
    N = native_lib
    valid = [e for _, e in c.encodings if E.expect_decode(e, False)[0] == E.OK]
    refused = [e for _, e in c.encodings if E.expect_decode(e, False)[0] != E.OK]
    n = len(valid)

    def run(encs):
        aff, bad = ctypes.create_string_buffer(96 * len(encs)), ctypes.c_size_t(0)
        rc = N.cg1_batch_decompress_pool(b"".join(encs), len(encs), None, aff, 0, ctypes.byref(bad))
        return rc, bad.value, aff.raw

    rc, _, aff = run(valid)
    assert rc == N.OK and [aff[96 * i: 96 * i + 96] for i in range(n)] == [E.expect_decode(e, False)[1] for e in valid]
    for t, e in enumerate(refused):
        for pos in (0, n // 2 + t % 5, n - 1):
            encs = list(valid)
            encs[pos] = e
            rc, bad, _ = run(encs)
            assert (rc, bad) == (status(N, E.expect_decode(e, False)[0]), pos), (e.hex(), pos)
    encs = list(valid)
    encs[n - 3], encs[7] = refused[0], refused[-1]
    assert run(encs)[:2] == (status(N, E.expect_decode(refused[-1], False)[0]), 7)


def test_host_compress_at_the_sign_boundary(native_lib, c):
    """cg1_compress and cg1_batch_compress on every boundary point and every other point the edge encodings decode to."""
    N = native_lib
    pts = c.boundary_pts + [p for p in c.valid_points if p not in c.boundary_pts] + [None]
    want = [O.g1_compress(p) for p in pts]
    assert set(c.inner_pts) <= set(pts) and sum(1 for w in want if w[0] & 0x20) >= 46 and sum(1 for w in want if not w[0] & 0x60) >= 46
    blobs = [blob_of(N, p) if p is not None else None for p in pts]
    ident = ctypes.create_string_buffer(N.POINT_BYTES)
    N.cg1_identity(ident)
    blobs[-1] = ident.raw
    for b, w in zip(blobs, want):
        out = ctypes.create_string_buffer(48)
        N.cg1_compress(out, b)
        assert out.raw == w
    out = ctypes.create_string_buffer(48 * len(pts))
    N.cg1_batch_compress(out, b"".join(blobs), len(pts))
    assert [out.raw[48 * i: 48 * i + 48] for i in range(len(pts))] == want


def test_host_validation_at_every_edge(native_lib, c):
    """cg1_validate_compressed (the Jacobi-symbol form of the unchecked decoder's decision): status class and identity flag."""
    N = native_lib
    for _, e in c.encodings:
        cls, raw = E.expect_decode(e, False)
        inf = ctypes.c_int(-1)
        assert N.cg1_validate_compressed(e, ctypes.byref(inf)) == status(N, cls), e.hex()
        if cls == E.OK:
            assert inf.value == (1 if raw == bytes(96) else 0), e.hex()


def test_host_subgroup_pool_on_small_orders(native_lib, c):
    """cg1_batch_subgroup_pool: 1 iff the oracle's [r]P is the identity, for points of order 3, 11, 10177, 859267, 52437899, their sums
    with points of G1, points of full order, their pure parts, and the boundary points."""
    N = native_lib
    pts = [p for _, p in c.subgroup]
    flags = ctypes.create_string_buffer(len(pts))
    assert N.cg1_batch_subgroup_pool(b"".join(E.raw96(p) for p in pts), len(pts), flags, 0) == N.OK
    want = [1 if E.in_g1(p) else 0 for p in pts]
    assert list(flags.raw) == want, [lab for (lab, _), g, w in zip(c.subgroup, flags.raw, want) if g != w]
    assert 7 <= sum(want) < len(want) - 50
