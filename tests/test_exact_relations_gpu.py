"""k_exact_relations (csrc/kernels_exact.h) through cg1_exact_relations_device: signed sums of at most four terms k * P over the WHOLE curve,
one launch for the whole case list of tests/exact_relation_cases.py.  Needs an MI355X.

The builder asserts, from a plain-int replay of the kernel's shared ladder, that the list drives it into every exceptional addition (P + P,
P - P, an identity accumulator revived, identity table entries of small-order bases met with a finite and with an identity accumulator, the
same around the "one" terms).  Expected verdicts are the oracle's; the host twin runs on the same arrays and must say the same."""
import ctypes
import struct

import pytest

import exact_relation_cases as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c():
    return X.cases()


@pytest.fixture(scope="module")
def dev(native_lib, c):
    """the context and the fixture's points and scalars on the device, uploaded once"""
    cx = native_lib.Context(0)
    d_pts, d_sc = cx.alloc(len(c.points96)), cx.alloc(len(c.scalars32))
    d_pts.upload(c.points96); d_sc.upload(c.scalars32)
    yield cx, d_pts, d_sc
    d_pts.free(); d_sc.free()
    cx.close()


def run_device(N, dev, c, terms):
    """-> the verdicts of ONE cg1_exact_relations_device call; the byte behind the last verdict must stay as it was"""
    cx, d_pts, d_sc = dev
    n = len(terms) // (8 * X.TERMS)
    d_ok = cx.alloc(n + 1)
    try:
        d_ok.upload(b"\xee" * (n + 1))
        cx.check(N.cg1_exact_relations_device(cx.handle, d_pts.ptr, len(c.points), d_sc.ptr, len(c.scalars), terms, n, d_ok.ptr))
        cx.check(N.cg1_stream_sync(cx.handle))
        out = d_ok.download()
    finally:
        d_ok.free()
    assert out[n:] == b"\xee" and set(out[:n]) <= {0, 1}
    return [bool(b) for b in out[:n]]


def host(N, c, terms):
    n = len(terms) // (8 * X.TERMS)
    ok = ctypes.create_string_buffer(n)
    assert N.cg1_exact_relations(c.points96, len(c.points), c.scalars32, len(c.scalars), terms, n, ok, 0) == 0
    return [bool(b) for b in ok.raw]


def test_device_equals_oracle_and_host_twin(native_lib, dev, c):
    got = run_device(native_lib, dev, c, c.terms)
    wrong = [(r[0], r[1], g) for r, g in zip(c.relations, got) if g != r[3]]
    assert not wrong, wrong[:8]
    assert got == host(native_lib, c, c.terms)


def test_reversed_order(native_lib, dev, c):
    n = len(c.relations)
    rev = b"".join(c.terms[32 * i: 32 * i + 32] for i in range(n - 1, -1, -1))
    assert run_device(native_lib, dev, c, rev) == c.want[::-1] == host(native_lib, c, rev)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_launch_geometry_edges(native_lib, dev, c, n):
    """a relation is a block of one wave: the counts around a full wave's worth of blocks, taken from the middle of the list so that every
    count holds both verdicts (n = 1: one relation that holds, then one that does not)"""
    lo = next(i for i in range(len(c.want) - 65) if c.want[i] and not c.want[i + 1])
    if n == 1:
        for i in (lo, lo + 1):
            assert run_device(native_lib, dev, c, c.terms[32 * i: 32 * i + 32]) == [c.want[i]]
        return
    assert run_device(native_lib, dev, c, c.terms[32 * lo: 32 * (lo + n)]) == c.want[lo: lo + n]
    assert len(set(c.want[lo: lo + n])) == 2


def test_bad_index_is_refused_before_the_launch(native_lib, dev, c):
    N = native_lib
    cx, d_pts, d_sc = dev
    none = struct.pack("<II", X.NONE_MARK, 0)
    d_ok = cx.alloc(4)
    try:
        d_ok.upload(b"\xee" * 4)
        for bad in (struct.pack("<II", len(c.points), X.ONE_MARK), struct.pack("<II", 0, len(c.scalars))):
            terms = c.terms[:32] + none * 3 + bad
            assert N.cg1_exact_relations_device(cx.handle, d_pts.ptr, len(c.points), d_sc.ptr, len(c.scalars), terms, 2, d_ok.ptr) == N.ERR_ARG
        cx.check(N.cg1_stream_sync(cx.handle))
        assert d_ok.download() == b"\xee" * 4                 # nothing ran
        assert N.cg1_exact_relations_device(cx.handle, d_pts.ptr, len(c.points), d_sc.ptr, len(c.scalars), None, 0, d_ok.ptr) == 0
    finally:
        d_ok.free()


def test_gather_blocks_with_a_cleared_range(native_lib, dev):
    """cg1_exact_gather_device: dst block j = src block idx[j] with a byte range zeroed; a stride of 0 repeats one block; what lies behind the
    last block stays; a bad index or size is refused before anything runs."""
    N = native_lib
    cx = dev[0]
    nblk, stride, block = 7, 72, 64                      # the source's blocks are 72 bytes apart, 64 bytes of each copied
    big = 1300                                            # the second call's destination stride
    src = bytes((i * 7 + 3) & 0xFF or 1 for i in range(nblk * stride))
    idx = [6, 0, 0, 3, 5]
    d_src, d_dst, d_big = cx.alloc(len(src)), cx.alloc(len(idx) * 80 + 8), cx.alloc(2 * big + 4)
    try:
        d_src.upload(src); d_dst.upload(b"\xee" * (len(idx) * 80 + 8)); d_big.upload(b"\xee" * (2 * big + 4))
        i32 = struct.pack("<%dI" % len(idx), *idx)
        cx.check(N.cg1_exact_gather_device(cx.handle, d_src.ptr, nblk, stride, i32, len(idx), d_dst.ptr, 80, block, 8, 12))
        cx.check(N.cg1_exact_gather_device(cx.handle, d_src.ptr, 1, 0, bytes(8), 2, d_big.ptr, big, 500, 0, 0))
        cx.check(N.cg1_stream_sync(cx.handle))
        out, out_big = d_dst.download(), d_big.download()
        for j, i in enumerate(idx):
            blk = src[i * stride: i * stride + block]
            assert out[80 * j: 80 * j + block] == blk[:8] + bytes(12) + blk[20:], j
            assert out[80 * j + block: 80 * j + 80] == b"\xee" * 16
        assert out[80 * len(idx):] == b"\xee" * 8
        assert out_big[:500] == src[:500] and out_big[big: big + 500] == src[:500] and out_big[500: big] == b"\xee" * (big - 500) and out_big[big + 500:] == b"\xee" * (big - 500 + 4)
        before = d_dst.download()
        for args in ((nblk, stride, struct.pack("<I", nblk), 1, 80, block, 0, 0),      # an index past the source
                     (nblk, stride, i32, len(idx), 80, block + 2, 0, 0),               # no multiple of 4
                     (nblk, stride, i32, len(idx), 60, block, 0, 0),                   # a block longer than the destination's stride
                     (nblk, stride, i32, len(idx), 80, 76, 0, 0),                      # ... than the source's
                     (nblk, stride, i32, len(idx), 80, block, 60, 8)):                 # a cleared range past the block
            assert N.cg1_exact_gather_device(cx.handle, d_src.ptr, args[0], args[1], args[2], args[3], d_dst.ptr, *args[4:]) == N.ERR_ARG, args
        cx.check(N.cg1_stream_sync(cx.handle))
        assert d_dst.download() == before
    finally:
        d_src.free(); d_dst.free(); d_big.free()
