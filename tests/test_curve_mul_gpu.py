"""Every device engine that multiplies or sums caller-supplied points, over the WHOLE curve (tests/curve_mul_cases.py).  Needs an MI355X.

The reference decodes points unchecked (util.py:35-36), so bases of order 3, 11, 10177, 859267, 52437899, 33, their sums with points of
G1 and the identity are legal inputs, and with them the ladders run into P + P, P - P, an identity accumulator in mid-ladder and table
entries that are the identity -- branches that multiples of the generator under canonical scalars never reach (the builder asserts, from
a plain-int trace of each ladder, that the case list does).  Every expected value is the oracle's integer double-and-add; every
comparison is byte for byte.  Each engine is forced with the context's own switches:
  k_batch_mul_row    cg1_batch_mul_add with "batch_mul_host_max" = 0                     (one wave per output, 4-bit digits)
  k_batch_mul_quad   ... and "batch_mul_row" = 0; cg1_batch_mul_add_device                 (one quad per output, 2-bit digits, {P, 2P, 3P})
  k_batch_mul        the same two calls with "batch_mul_quad_max" = 0                      (one lane per output, bit by bit)
  the host's pool    cg1_batch_mul_add_pool, the twin
  cg1_lincomb_batch  path 1, and path 0 with the row kernel, the quad kernel and the lane kernel taking the map / fold outputs
  k_batch_sum        cg1_batch_sum and cg1_batch_sum_device
  k_msm_small, the regime-A chain ("small_msm" = 0), the batched single launch and the regime-B chain, all with "glv" = 0
Before k_batch_mul_quad's table knew that 3P may be the identity, the quad cases failed at the bases of order 3 (76 of the 168 pairs of
+-T3 with a scalar, 7 and 13 among them).  The whole file takes 2 s on an MI355X, half of it the fixture; no test takes 0.1 s."""
import contextlib
import ctypes
import random

import pytest

import codec_edge_cases as E
import curve_mul_cases as M
from conftest import from_raw96
from oracle import bls12_381 as O
from oracle import c_oracle as C

pytestmark = pytest.mark.gpu
DEFAULTS = {"batch_mul_host_max": -1, "batch_mul_row": 1, "batch_mul_quad_max": 8192, "small_msm": 1}      # csrc/host_context.h
# engine -> (entry point, the switches that force it)
ENGINES = {
    "pool": ("pool", {}),
    "row": ("host", {"batch_mul_host_max": 0}),
    "quad_host": ("host", {"batch_mul_host_max": 0, "batch_mul_row": 0}),
    "quad_device": ("device", {}),
    "lane_host": ("host", {"batch_mul_host_max": 0, "batch_mul_row": 0, "batch_mul_quad_max": 0}),
    "lane_device": ("device", {"batch_mul_quad_max": 0}),
}


@pytest.fixture(scope="module")
def c():
    return M.cases()


@pytest.fixture(scope="module")
def ctx(native_lib):
    cx = native_lib.Context(0)
    yield cx
    cx.close()


@contextlib.contextmanager
def forced(ctx, params):
    try:
        for name, value in params.items():
            ctx.set_param(name, value)
        yield
    finally:
        for name in params:
            ctx.set_param(name, DEFAULTS[name])


def batch_mul(N, ctx, engine, bases96, nbase, sc32, nscalars, addend96, n):
    """out[i] = addend[i] + scalars[i % nscalars] * bases[i % nbase] on the engine -> n affine96 records; the device entry writes into a
    buffer pre-filled with 0xEE and must leave what follows record n - 1 alone."""
    entry, params = ENGINES[engine]
    with forced(ctx, params):
        if entry == "pool":
            out = ctypes.create_string_buffer(96 * n)
            assert N.cg1_batch_mul_add_pool(bases96, nbase, sc32, nscalars, addend96, out, n, 0) == N.OK
            return out.raw
        if entry == "host":
            return ctx.batch_mul_add_host(bases96, nbase, sc32, nscalars, addend96, n)
        bufs = [ctx.alloc(96 * nbase), ctx.alloc(32 * nscalars), ctx.alloc(96 * n + 96)] + ([ctx.alloc(96 * n)] if addend96 is not None else [])
        try:
            bufs[0].upload(bases96[: 96 * nbase]); bufs[1].upload(sc32[: 32 * nscalars]); bufs[2].upload(b"\xee" * (96 * n + 96))
            if addend96 is not None:
                bufs[3].upload(addend96)
            ctx.check(N.cg1_batch_mul_add_device(ctx.handle, bufs[0].ptr, nbase, bufs[1].ptr, nscalars, bufs[3].ptr if addend96 is not None else None,
                                                 bufs[2].ptr, n))
            out = bufs[2].download()
        finally:
            for b in bufs:
                b.free()
        assert out[96 * n:] == b"\xee" * 96
        return out[: 96 * n]


def run_cases(N, ctx, c, engine, cases, with_addend, tag):
    n = len(cases)
    got = batch_mul(N, ctx, engine, b"".join(E.raw96(c.bases[m[0]][1]) for m in cases), n, b"".join(M.s32(m[1]) for m in cases), n,
                    b"".join(E.raw96(m[3]) for m in cases) if with_addend else None, n)
    bad = [(i, c.bases[m[0]][0], hex(m[1]), m[2]) for i, m in enumerate(cases) if got[96 * i: 96 * i + 96] != E.raw96(m[4] if with_addend else c.want(m[0], m[1]))]
    assert not bad, (engine, tag, len(bad), bad[:12])


def head_cases(c):
    """The cases that lead every small launch: order 3 under the radix-4 digits 3 1, 1 3, 3 3, 1 1 (13, 7, 15, 5) and 3, order 33, 11."""
    pick = lambda label, k: next(m for m in c.mul if c.bases[m[0]][0] == label and m[1] == k and m[2] != "none")
    return [pick("t3", 13), pick("t3", 7), pick("-t3", 13), pick("t3", 15), pick("t3", 5), pick("t3", 3), pick("t3 + order 11", 15),
            pick("order 11", 12), pick("-t3", 7), pick("t3 + g1", 13), pick("identity", 7), pick("g1 a", O.R + 1)]


@pytest.mark.parametrize("engine", list(ENGINES))
def test_engines_at_block_edges(native_lib, ctx, c, engine):
    """n = 1, 15, 16, 17, 63, 64, 65 (16 quads per block, whole quads leave together) and 127, 128, 129 (128 lanes per block), with and
    without the addend array; the first lanes and the LAST lane hold order-3 cases."""
    N = native_lib
    rng = random.Random(0xED6E)
    head = head_cases(c)
    rest = [m for m in c.mul if m[2] != "none"]
    for n in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129):
        cases = (head + rng.sample(rest, n))[:n]
        if n > 1:
            cases[-1] = head[1]
        for with_addend in (False, True):
            run_cases(N, ctx, c, engine, cases, with_addend, n)


@pytest.mark.parametrize("engine", list(ENGINES))
def test_whole_case_list_in_one_shuffled_launch(native_lib, ctx, c, engine):
    """Every (base, scalar) pair in one launch, shuffled: neighbouring lanes of a wave hold scalars of different bit lengths (the leading
    zero skip diverges per lane) and take different exceptional branches.  Once without addends, once as A + s * B."""
    N = native_lib
    rng = random.Random(0x5AFF1E)
    plain = [m for m in c.mul if m[2] == "none"]
    rng.shuffle(plain)
    run_cases(N, ctx, c, engine, plain, False, "plain")
    fold = list(c.mul)                                      # ("none": the identity as its addend record)
    rng.shuffle(fold)
    run_cases(N, ctx, c, engine, fold, True, "fold")


@pytest.mark.parametrize("engine", list(ENGINES))
def test_modular_indexing(native_lib, ctx, c, engine):
    """nbase = 1, nscalars = 1, and counts that do not divide n: out[i] = scalars[i % nscalars] * bases[i % nbase]."""
    N = native_lib
    bases96 = b"".join(E.raw96(pt) for _, pt, _ in c.bases)
    sc32 = b"".join(M.s32(k) for k in c.scalars)
    for b0, nbase, k0, nscalars, n in M.index_shapes(c):
        got = batch_mul(N, ctx, engine, bases96[96 * b0: 96 * (b0 + nbase)], nbase, sc32[32 * k0: 32 * (k0 + nscalars)], nscalars, None, n)
        bad = [i for i in range(n) if got[96 * i: 96 * i + 96] != E.raw96(c.want(b0 + i % nbase, c.scalars[k0 + i % nscalars]))]
        assert not bad, (engine, b0, nbase, k0, nscalars, bad[:12])


@pytest.mark.parametrize("label,path,params", [("pool", 1, {}), ("row", 0, {}), ("quad", 0, {"batch_mul_row": 0}),
                                               ("lane", 0, {"batch_mul_row": 0, "batch_mul_quad_max": 0})])
def test_lincomb_batch_against_the_oracle(native_lib, ctx, c, label, path, params):
    """Map (s * B, s * (-B)), fold (A + s * B) and four-to-six-term combinations in one batch: path 1 (the pool), and path 0 with the
    map / fold outputs on k_batch_mul_row, on k_batch_mul_quad and on k_batch_mul (without the row kernel path 0 hands them to the device
    from 2 048 on: the batch holds more)."""
    N = native_lib
    lb, offsets, tb, ls, want = c.lincomb
    n_out = len(want)
    shaped = sum(1 for j in range(n_out) if offsets[j + 1] - offsets[j] <= 2 and sum(1 for k in ls[offsets[j]: offsets[j + 1]] if k > 1) == 1)
    assert 2048 <= shaped <= 4096
    ob, oa, ok = ctypes.create_string_buffer(144 * n_out), ctypes.create_string_buffer(96 * n_out), ctypes.create_string_buffer(48 * n_out)
    used = ctypes.c_int(0)
    with forced(ctx, params):
        ctx.check(N.cg1_lincomb_batch(ctx.handle, b"".join(E.raw96(p) for p in lb), len(lb), (ctypes.c_uint32 * (n_out + 1))(*offsets), n_out,
                                      (ctypes.c_uint32 * len(tb))(*tb), b"".join(M.s32(k) for k in ls), path, ob, oa, ok, ctypes.byref(used)))
    assert used.value == (1 if path == 1 else 2)
    aff = ctypes.create_string_buffer(96 * n_out)
    N.cg1_batch_to_affine96(aff, ob.raw, n_out)
    bad = [j for j, w in enumerate(want) if not (oa.raw[96 * j: 96 * j + 96] == aff.raw[96 * j: 96 * j + 96] == E.raw96(w)
                                                 and ok.raw[48 * j: 48 * j + 48] == O.g1_compress(w))]
    assert not bad, (label, len(bad), [(j, [(t & 0x7FFFFFFF, t >> 31, hex(k)) for t, k in zip(tb[offsets[j]: offsets[j + 1]], ls[offsets[j]: offsets[j + 1]])]) for j in bad[:8]])


@pytest.mark.parametrize("entry", ["host", "device"])
def test_batch_sum(native_lib, ctx, c, entry):
    """[T3] * 2, * 3, * 64, * 129, [P, -P, Q], an empty group, and groups of 1, 63, 64, 65, 129 entries that put identity partial sums,
    equal and opposite sums into the 64-lane shuffle tree (curve_mul_cases.tree_events says which)."""
    N = native_lib
    for groups in (c.sums, c.sums[::-1]):
        offsets, pts = [0], []
        for _, g, _ in groups:
            pts += g
            offsets.append(len(pts))
        p96, m = b"".join(E.raw96(p) for p in pts), len(groups)
        if entry == "host":
            got = ctx.batch_sum_host(p96, offsets)
        else:
            d_p, d_o = ctx.alloc(len(p96)), ctx.alloc(96 * m + 96)
            try:
                d_p.upload(p96); d_o.upload(b"\xee" * (96 * m + 96))
                ctx.check(N.cg1_batch_sum_device(ctx.handle, d_p.ptr, (ctypes.c_uint32 * (m + 1))(*offsets), m, d_o.ptr))
                got = d_o.download()
            finally:
                d_p.free(); d_o.free()
            assert got[96 * m:] == b"\xee" * 96
        bad = [label for j, (label, _, w) in enumerate(groups) if got[96 * j: 96 * j + 96] != E.raw96(w)]
        assert not bad, (entry, bad)


def affine_of(N, blob):
    out = ctypes.create_string_buffer(96)
    N.cg1_to_affine96(out, blob)
    return out.raw


@pytest.fixture(scope="module")
def msm_input(ctx, c):
    pts, ks, total = c.msm
    p96, s32 = b"".join(E.raw96(p) for p in pts), b"".join(M.s32(k) for k in ks)
    d_p, d_s = ctx.alloc(len(p96)), ctx.alloc(len(s32))
    d_p.upload(p96); d_s.upload(s32)
    yield p96, s32, d_p, d_s, len(pts), E.raw96(total)
    d_p.free(); d_s.free()


@pytest.mark.parametrize("small,window_c", [(1, 0), (1, 4), (1, 7), (1, 9), (0, 0), (0, 8), (0, -7)])
def test_msm_over_the_whole_curve(native_lib, ctx, msm_input, small, window_c):
    """~300 terms over bases of every small order, repeats and both signs of each (buckets hold P + P and P - P), scalars below 2^255
    as plain integers, "glv" = 0: k_msm_small (one launch) and the regime-A chain give the oracle's sum."""
    N = native_lib
    _, _, d_p, d_s, n, want = msm_input
    with forced(ctx, {"small_msm": small}):
        got = ctx.msm_device(d_p, d_s, n, window_c=window_c)
        assert ctx.last_counts()["accumulate_launches"] == (0 if small else 1)
    assert affine_of(N, got) == want


@pytest.mark.parametrize("small", [1, 0])
def test_batched_msm_over_the_whole_curve(native_lib, ctx, msm_input, small):
    """The same input cut into 20 MSMs, one of them empty: as one k_msm_small launch (20 MSMs of these sizes fit it) and, with
    "small_msm" = 0, on the regime-B chain.  Each against the C oracle (tests/test_curve_mul.py: the oracle's sum on the whole input),
    and their sum against the oracle's."""
    N = native_lib
    p96, s32, d_p, d_s, n, want = msm_input
    rng = random.Random(0xB)
    cuts = sorted(rng.sample(range(1, n), 18))
    offsets = [0] + cuts[:7] + [cuts[6]] + cuts[7:] + [n]
    assert len(offsets) == 21
    with forced(ctx, {"small_msm": small}):
        got = ctx.msm_batched_device(d_p, d_s, offsets)
    total = None
    for j, blob in enumerate(got):
        lo, hi = offsets[j], offsets[j + 1]
        a = affine_of(N, blob)
        ref = C.compress(C.msm_bucket(p96[96 * lo: 96 * hi], s32[32 * lo: 32 * hi], hi - lo)) if hi > lo else O.g1_compress(None)
        assert O.g1_compress(from_raw96(a)) == ref, (small, j, lo, hi)
        total = O.g1_add(total, from_raw96(a))
    assert E.raw96(total) == want
