"""A buffer a context keeps between calls fails to grow: the call is refused, the group it was growing is left EMPTY (pointers null,
capacity zero), and the next call -- a smaller one that the stale capacity would have let through, then the refused one again -- gives
the right bytes.  Needs an MI355X.

The failure is injected (context parameter "alloc_fail_at" = k: the k-th allocation the growth helper attempts on that context fails
as out of memory without reaching the runtime), so nothing here exhausts the card, and a refused call returns before it launches
anything on the buffer that did not grow.  Every scenario walks k = 1, 2, ... over a fresh context (or a fresh table) until the big
call's allocations are exhausted; results are pinned to the C oracle (oracle.c_oracle), the recorded reference bytes or the host twin."""
import random
import types

import pytest

from conftest import raw96
from oracle import bls12_381 as O
from oracle import c_oracle as C
from test_msm_gpu import compress_blob

pytestmark = pytest.mark.gpu

K_MAX = 64


def walk(arm, small, big, check_big, min_failing, fresh, close, unchanged=None):
    """The loop every scenario shares.  fresh() -> a state with nothing grown yet; small(state) -> bytes; big(state) -> results, or
    NativeError when the armed allocation is one of its own; check_big(results) asserts them against the oracle; arm(state, k) sets
    "alloc_fail_at"; unchanged(state): what else a refused call must have left alone."""
    from curdleproofs_pie_amd._native import NativeError

    failing = 0
    for k in range(1, K_MAX + 2):
        assert k <= K_MAX, "the big call never ran out of allocations to fail"
        state = fresh()
        try:
            before = small(state)
            arm(state, k)
            try:
                results = big(state)
            except NativeError as e:
                assert "injected" in str(e), str(e)
                failing += 1
                if unchanged is not None:
                    unchanged(state)
                assert small(state) == before, k            # (the injection has fired: it is disarmed)
                arm(state, 0)
                check_big(big(state))
                continue
            check_big(results)
            arm(state, 0)
            break
        finally:
            arm(state, 0)
            close(state)
    assert failing >= min_failing, (failing, k)


@pytest.fixture(scope="module")
def terms(native_lib):
    """6 000 terms over a cycle of 20 oracle-made bases, and the oracle's MSM over their first n (computed once per n)."""
    rng = random.Random(4077)
    pts = [raw96(O.g1_mul(O.G1_GEN, rng.randint(1, O.R - 1))) for _ in range(20)]
    n = 6000
    t = types.SimpleNamespace(p96=b"".join(pts[i % 20] for i in range(n)), s32=b"".join(rng.randint(0, O.R - 1).to_bytes(32, "little") for _ in range(n)), memo={})

    def want(lo, hi):
        if (lo, hi) not in t.memo:
            t.memo[lo, hi] = C.compress(C.msm_bucket(t.p96[96 * lo: 96 * hi], t.s32[32 * lo: 32 * hi], hi - lo))
        return t.memo[lo, hi]

    t.want = want
    return t


def on_context(N, terms, n_max, **params):
    """fresh / close / arm over a new Context holding the first n_max terms on the device."""
    def fresh():
        ctx = N.Context(0)
        for name, v in params.items():
            ctx.set_param(name, v)
        dp, ds = ctx.alloc(96 * n_max), ctx.alloc(32 * n_max)
        dp.upload(terms.p96[:96 * n_max]); ds.upload(terms.s32[:32 * n_max])
        return types.SimpleNamespace(ctx=ctx, dp=dp, ds=ds)

    def close(s):
        s.dp.free(); s.ds.free(); s.ctx.close()

    return dict(fresh=fresh, close=close, arm=lambda s, k: s.ctx.set_param("alloc_fail_at", k))


def test_regime_a_chain(native_lib, terms):
    """ensure(): 2 100 terms at c = 8 (above SM_MAX_N = 2 048: the chain, not k_msm_small), then 5 000 at the balanced plan of width 12 --
    more terms, wider windows: the points, the per-bucket group (cap_nb), the zero block, the sort's per-entry and per-slice buffers --
    then 5 000 at c = 5 -- more windows: the per-window groups (cap_bigflag, cap_blockcnt, cap_partial, cap_out) and the entries."""
    N = native_lib
    msm = lambda s, n, c: compress_blob(N, s.ctx.msm_device(s.dp, s.ds, n, window_c=c))

    def check(res):
        assert res == [terms.want(0, 5000)] * 2

    walk(small=lambda s: msm(s, 2100, 8), big=lambda s: [msm(s, 5000, -12), msm(s, 5000, 5)], check_big=check, min_failing=12,
         **on_context(N, terms, 5000))
    assert msm_once(N, terms, 2100, 8) == terms.want(0, 2100)


def msm_once(N, terms, n, c):
    ctx = N.Context(0)
    try:
        dp, ds = ctx.alloc(96 * n), ctx.alloc(32 * n)
        dp.upload(terms.p96[:96 * n]); ds.upload(terms.s32[:32 * n])
        return compress_blob(N, ctx.msm_device(dp, ds, n, window_c=c))
    finally:
        ctx.close()


@pytest.mark.parametrize("m_small,m_big,horner", [(6, 30, "device"), (2, 6, "host")])
def test_regime_b(native_lib, terms, m_small, m_big, horner):
    """batched_chain_enqueue with "small_msm" = 0: MSMs of 10 terms, then more MSMs of 40 -- ensure()'s groups and the batch's own:
    d_boffs, d_gsum, d_bout / h_bout with more than 24 MSMs (the device Horner), d_gout / h_gout up to 24 (the host Horner)."""
    N = native_lib
    assert (m_big <= 24) == (horner == "host")

    def batched(s, m, n):
        offs = [n * j for j in range(m + 1)]
        return [compress_blob(N, b) for b in s.ctx.msm_batched_device(s.dp, s.ds, offs)]

    def check(res):
        assert res == [terms.want(40 * j, 40 * j + 40) for j in range(m_big)]

    walk(small=lambda s: batched(s, m_small, 10), big=lambda s: batched(s, m_big, 40), check_big=check, min_failing=3,
         **on_context(N, terms, 40 * m_big, small_msm=0))


def test_single_launch_msm(native_lib, terms):
    """k_msm_small: 100 terms (one slice: no partial sums), then 600 (three slices: d_small_partial grows)."""
    N = native_lib
    msm = lambda s, n: compress_blob(N, s.ctx.msm_device(s.dp, s.ds, n))

    def check(res):
        assert res == terms.want(0, 600)

    walk(small=lambda s: msm(s, 100), big=lambda s: msm(s, 600), check_big=check, min_failing=1, **on_context(N, terms, 600))
    assert terms.want(0, 100) == msm_once(N, terms, 100, 0)


def test_host_pointer_msm(native_lib, terms):
    """cg1_msm: 100 terms through the mapped h_lin, then 4 200 (above 4 096: staged through ensure_stage, and regime A behind it), then
    6 000 (both staging buffers again, and the chain's per-term buffers)."""
    N = native_lib
    msm = lambda s, n: compress_blob(N, s.ctx.msm_host(terms.p96, terms.s32, n))

    def check(res):
        assert res == [terms.want(0, 4200), terms.want(0, 6000)]

    def small(s):
        got = msm(s, 100)
        assert got == terms.want(0, 100)
        return got

    walk(small=small, big=lambda s: [msm(s, 4200), msm(s, 6000)], check_big=check, min_failing=2, **on_context(N, terms, 1))


def on_default_context(N):
    return lambda s, k: N.default_context().set_param("alloc_fail_at", k)


def test_fixed_table_msm_many(native_lib):
    """FixedBaseTable.msm_many: two MSMs of 8 terms (the staging block h_in / d_in at its 64 KiB floor), then 40 of 65 (94 KB: it grows,
    and so do the partial sums of the sliced MSMs).  The table allocates through its context: the default context is the one armed."""
    from curdleproofs_pie_amd import G1Point, Scalar
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable

    N = native_lib
    rng = random.Random(881)
    raws = [O.g1_mul(O.G1_GEN, rng.randint(1, O.R - 1)) for _ in range(12)]
    p96 = [raw96(p) for p in raws]
    objs = [G1Point.from_compressed_bytes_unchecked(O.g1_compress(p)) for p in raws]

    def jobs(m, n):                                                      # m MSMs of n terms: (table indices, scalars as ints), the same at every call
        r = random.Random(m)
        return [([(7 * j + i) % 12 for i in range(n)], [r.randint(0, O.R - 1) for _ in range(n)]) for j in range(m)]

    def run(tab, m, n):
        return [bytes(p.to_compressed_bytes()) for p in tab.msm_many([(idx, [Scalar(v) for v in sc]) for idx, sc in jobs(m, n)])]

    want = {(m, n): [C.compress(C.compute_msm(b"".join(p96[i] for i in idx), b"".join(v.to_bytes(32, "little") for v in sc), n)) for idx, sc in jobs(m, n)]
            for m, n in ((2, 8), (40, 65))}

    def small(tab):
        got = run(tab, 2, 8)
        assert got == want[2, 8]
        return got

    def check(res):
        assert res == want[40, 65]

    walk(arm=on_default_context(N), small=small, big=lambda tab: run(tab, 40, 65), check_big=check, min_failing=1,
         fresh=lambda: FixedBaseTable(objs), close=lambda tab: tab.close())


def test_ipa_chain_staging(native_lib):
    """ipa_prove_device at n = 8 for one prover (the fixture's bytes), then four in step: the chain's staging block (h_chain / d_chain)
    grows.  The refused call leaves every transcript where it was; the four provers get what the host-driven path gives them."""
    import json
    import os

    import test_ipa_device_gpu as T
    from curdleproofs_pie_amd.prover_kernels import ipa_prove_device, ipa_prove_device_many

    N = native_lib
    case = json.load(open(os.path.join(T.ROOT, "tests", "golden", "ipa_device_vectors.json")))["cases"][1]
    prefix = lambda i: None if i == 0 else b"prover %d" % i
    ref = T.Case(case)
    assert ref.n == 8
    try:
        want = []
        for i in range(4):
            t = ref.transcript(prefix(i))
            want.append((T.to_bytes(T.host_driven(ref.table, *ref.prover(rot=i)[:10], t, ref.coeffs)), T.state(t)))
    finally:
        ref.table.close()
    assert want[0][0].hex() == case["proof"]

    def fresh():
        k = T.Case(case)
        k.ts = None
        return k

    def small(k):
        got = T.to_bytes(ipa_prove_device(k.table, *k.prover()[:10], k.transcript(), G_prime_coeffs=k.coeffs))
        assert got.hex() == case["proof"]
        return got

    def big(k):
        k.ts = [k.transcript(prefix(i)) for i in range(4)]
        got = ipa_prove_device_many(k.table, [k.prover(rot=i) for i in range(4)], k.ts)
        return [(T.to_bytes(g), T.state(t)) for g, t in zip(got, k.ts)]

    def unchanged(k):
        assert [T.state(t) for t in k.ts] == [T.state(k.transcript(prefix(i))) for i in range(4)]

    def check(res):
        assert res == want

    walk(arm=on_default_context(N), small=small, big=big, check_big=check, min_failing=1, fresh=fresh, close=lambda k: k.table.close(),
         unchanged=unchanged)


def test_tracker_scan_table(native_lib):
    """300 trackers against 40 secrets (more than 32: the tables route) on a context that has not scanned yet: the tile's table is the
    first allocation, refused; the same scan unarmed equals the host twin (cg1_tracker_match), planted matches included."""
    from test_tracker_scan import native_match

    N = native_lib
    rng = random.Random(5150)
    ks = [rng.randint(1, O.R - 1) for _ in range(40)]
    pairs = []
    for i in range(20):                                                  # a cycle of 20 trackers; every fourth opens under one of the secrets
        r_G = O.g1_mul(O.G1_GEN, rng.randint(1, O.R - 1))
        k = ks[(7 * i) % 40] if i % 4 == 0 else rng.randint(1, O.R - 1)
        pairs.append(O.g1_compress(r_G) + O.g1_compress(O.g1_mul(r_G, k)))
    T, V = 300, 40
    c = types.SimpleNamespace(trackers=[None] * T, ks=ks, words=1, tile=0, trackers96=b"".join(pairs[i % 20] for i in range(T)),
                              ks32=b"".join(k.to_bytes(32, "little") for k in ks))
    host = native_match(N, c)
    assert any(host[0][8 * i: 8 * i + 8] != bytes(8) for i in range(T)) and host[1] == [0] * T and host[2] == [0] * V
    ctx = N.Context(0)
    try:
        ctx.set_param("alloc_fail_at", 1)
        with pytest.raises(N.NativeError, match="injected"):
            native_or_raise(N, c, ctx)
        ctx.set_param("alloc_fail_at", 0)
        assert native_match(N, c, ctx) == host
    finally:
        ctx.close()


def native_or_raise(N, c, ctx):
    import ctypes

    T, V = len(c.trackers), len(c.ks)
    bm = ctypes.create_string_buffer(8 * c.words * T)
    ts, kst = (ctypes.c_int32 * T)(), (ctypes.c_int32 * V)()
    ctx.check(N.cg1_tracker_match_device(ctx.handle, c.trackers96, T, c.ks32, V, c.tile, bm, ts, kst))
