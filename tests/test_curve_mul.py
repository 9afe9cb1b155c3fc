"""The host's scalar-multiplication engines over the whole curve (tests/curve_mul_cases.py): cg1_mul, the worker pool's batched
A + s * B (cg1_batch_mul_add_pool), its linear combinations (cg1_lincomb_batch_pool) and the host MSM (one combination of ~300 terms on
the pool) against the oracle's integer double-and-add, byte for byte: bases of order 3, 11, 10177, 859267, 52437899 and 33, their sums
with points of G1, the identity, 256-bit scalars taken as they stand.  No GPU: these are the host twins of what
tests/test_curve_mul_gpu.py asks of the device, and the first check of the fixture itself."""
import ctypes

import pytest

import codec_edge_cases as E
import curve_mul_cases as M
from oracle import bls12_381 as O
from oracle import c_oracle as C


@pytest.fixture(scope="module")
def c():
    return M.cases()


def test_the_fixture_is_what_it_says(c):
    """Every base of the issue's list with its order, every scalar class, and the ladders' exceptional branches reached (cases() itself
    asserts them; here the model that finds them is checked where its answer is known)."""
    orders = sorted(order for _, _, order in c.bases)
    assert orders == sorted([1, O.R, O.R, 3, 3, 11, 10177, 859267, 52437899, 3 * O.R, 11 * O.R, 33])
    assert {0, 1, 2, 3, 7, 13, (1 << 256) - 1, 1 << 255, O.R - 1, O.R, O.R + 1, 2 * O.R} <= set(c.scalars)
    assert len(c.pairs) == len(c.bases) * len(c.scalars) and len(c.mul) == 2 * len(c.pairs)
    # order 3, radix 4: 7 = (1, 3) adds the identity entry to a finite accumulator, 13 = (3, 1) to the identity and then P to it;
    # binary: 5 = 101 doubles (2 * 2P = P, + P), 3 = 11 cancels (2P + P), 7 revives the identity
    assert M.ladder_events(3, 7, 2) == ({"identity entry, acc finite"}, 1) and M.ladder_events(3, 13, 2) == ({"identity entry, acc identity"}, 1)
    assert M.ladder_events(3, 5, 1)[0] == {"acc == T"} and M.ladder_events(3, 3, 1) == ({"acc == -T"}, 0)
    assert M.ladder_events(3, 7, 1) == ({"acc == -T", "identity acc revived"}, 1)
    assert M.ladder_events(O.R, O.R - 1, 2)[0] == set()                 # a prime-order base under a canonical scalar meets none of them
    for w, required in M.REQUIRED_EVENTS.items():
        assert all(c.events[w][e] > 0 for e in required)
    assert all(c.sum_events[e] > 0 for e in M.TREE_EVENTS)
    # the oracle's own g1_mul agrees wherever it applies (a base of G1: the value mod r)
    for b in (1, 2):
        for k in c.scalars[::7]:
            assert O.g1_mul(c.bases[b][1], k % O.R) == c.want(b, k)


def test_cg1_mul(native_lib, c):
    N = native_lib
    for b, k in c.pairs:
        blob, out, aff = ctypes.create_string_buffer(144), ctypes.create_string_buffer(144), ctypes.create_string_buffer(96)
        assert N.cg1_from_affine96(blob, E.raw96(c.bases[b][1]), 1) == N.OK
        N.cg1_mul(out, blob.raw, M.s32(k))
        N.cg1_to_affine96(aff, out.raw)
        assert aff.raw == E.raw96(c.want(b, k)), (c.bases[b][0], hex(k))


def test_batch_mul_add_pool(native_lib, c):
    """Without an addend array, and A + s * B with A the identity, + s B (the addition doubles), - s B (it cancels), an unrelated point;
    then the modular indexing: one base, one scalar, a base count that does not divide n."""
    N = native_lib
    plain = [m for m in c.mul if m[2] == "none"]
    for cases, with_addend in ((plain, False), (c.mul, True)):
        n = len(cases)
        out = ctypes.create_string_buffer(96 * n)
        assert N.cg1_batch_mul_add_pool(b"".join(E.raw96(c.bases[m[0]][1]) for m in cases), n, b"".join(M.s32(m[1]) for m in cases), n,
                                        b"".join(E.raw96(m[3]) for m in cases) if with_addend else None, out, n, 0) == N.OK
        for i, m in enumerate(cases):
            assert out.raw[96 * i: 96 * i + 96] == E.raw96(m[4]), (c.bases[m[0]][0], hex(m[1]), m[2])
    bases96 = b"".join(E.raw96(pt) for _, pt, _ in c.bases)
    sc32 = b"".join(M.s32(k) for k in c.scalars)
    for b0, nbase, k0, nscalars, n in M.index_shapes(c):
        out = ctypes.create_string_buffer(96 * n)
        assert N.cg1_batch_mul_add_pool(bases96[96 * b0:], nbase, sc32[32 * k0:], nscalars, None, out, n, 0) == N.OK
        for i in range(n):
            assert out.raw[96 * i: 96 * i + 96] == E.raw96(c.want(b0 + i % nbase, c.scalars[k0 + i % nscalars])), (b0, nbase, k0, nscalars, i)


def test_lincomb_batch_pool(native_lib, c):
    N = native_lib
    lb, offsets, tb, ls, want = c.lincomb
    n_out = len(want)
    ob, oa, ok = ctypes.create_string_buffer(144 * n_out), ctypes.create_string_buffer(96 * n_out), ctypes.create_string_buffer(48 * n_out)
    assert N.cg1_lincomb_batch_pool(b"".join(E.raw96(p) for p in lb), len(lb), (ctypes.c_uint32 * (n_out + 1))(*offsets), n_out,
                                    (ctypes.c_uint32 * len(tb))(*tb), b"".join(M.s32(k) for k in ls), ob, oa, ok, 0) == N.OK
    aff = ctypes.create_string_buffer(96)
    for j, w in enumerate(want):
        assert oa.raw[96 * j: 96 * j + 96] == E.raw96(w) and ok.raw[48 * j: 48 * j + 48] == O.g1_compress(w), (j, offsets[j], offsets[j + 1])
        N.cg1_to_affine96(aff, ob.raw[144 * j: 144 * j + 144])
        assert aff.raw == E.raw96(w), j


def test_host_msm(native_lib, c):
    """The product's host path for an MSM: one combination of all the terms on the pool (what the Python face's deferred layer runs without
    a GPU); the C oracle the GPU tests elsewhere compare against gives the same point."""
    N = native_lib
    pts, ks, total = c.msm
    n = len(pts)
    assert n == 300 and all(k < 1 << 255 for k in ks) and total is not None
    p96, s32 = b"".join(E.raw96(p) for p in pts), b"".join(M.s32(k) for k in ks)
    oa = ctypes.create_string_buffer(96)
    assert N.cg1_lincomb_batch_pool(p96, n, (ctypes.c_uint32 * 2)(0, n), 1, (ctypes.c_uint32 * n)(*range(n)), s32, None, oa, None, 0) == N.OK
    assert oa.raw == E.raw96(total)
    assert C.compress(C.msm_bucket(p96, s32, n)) == O.g1_compress(total)
