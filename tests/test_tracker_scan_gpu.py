"""The tracker scan on the GPU: cg1_tracker_match_device (csrc/kernels_tracker_scan.h: light tables in tiles, one lane per pair) over the
cases of tests/tracker_scan_cases.py -- the oracle's bitmaps word for word, the statuses, and the host twin bit for bit -- down BOTH
routes of the device call (the tables for every case, whatever its number of secrets; one ladder per pair for every case; and the
default rule that chooses by the number of secrets), then tile edges beyond the cases' own, the timed mode, the refusals and the Python
face on the device."""
import ctypes

import pytest

import tracker_scan_cases as S
from test_tracker_scan import NAMES, native_match, pairs_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cs():
    return S.cases()


@pytest.fixture(scope="module")
def env(native_lib):
    return native_lib, native_lib.default_context()


ROUTES = {"tables": 0, "ladders": 1024, "default": 32}          # the context parameter "tracker_scan_ladder_max_ks"


@pytest.fixture(params=list(ROUTES))
def route(request, env):
    _, ctx = env
    ctx.set_param("tracker_scan_ladder_max_ks", ROUTES[request.param])
    yield request.param
    ctx.set_param("tracker_scan_ladder_max_ks", ROUTES["default"])


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_oracle_and_host_twin(env, cs, name, route):
    N, ctx = env
    c = cs[name]
    got = native_match(N, c, ctx)
    assert got[1] == c.tracker_status and got[2] == c.k_status
    assert got[0] == c.bitmap
    assert got == native_match(N, c)


def test_the_default_rule_takes_both_routes(env, cs):
    """Up to 32 secrets the timed call reports no table build, beyond it one."""
    N, ctx = env
    ms = (ctypes.c_float * 2)()
    ctx.set_param("tracker_scan_timing", 1)
    try:
        for name, built in (("scalars and identities", False), ("whole curve", True)):
            c = cs[name]
            assert (len(c.ks) > 32) == built
            assert native_match(N, c, ctx) == (c.bitmap, c.tracker_status, c.k_status)
            assert N.cg1_tracker_match_last_ms(ctx.handle, ms) == N.OK and (ms[0] > 0) == built and ms[1] > 0
    finally:
        ctx.set_param("tracker_scan_timing", 0)


@pytest.mark.parametrize("tile", [1, 2, 3, 5, 16, 17, 4096])
def test_every_tile_edge_gives_the_same_words(env, cs, tile):
    """A tile of one tracker, tiles that end inside the list, the list as one tile and a tile larger than the list, over the cases whose
    rows differ most: small orders (identity records), bad encodings (zero rows between live ones), the planted shapes."""
    N, ctx = env
    ctx.set_param("tracker_scan_ladder_max_ks", 0)                   # (bad encodings has two secrets: the tables all the same)
    try:
        for name in ("whole curve", "bad encodings", "5 x 64, tile 2", "differential 16 x 130"):
            c = cs[name]
            assert native_match(N, c, ctx, tile=tile) == (c.bitmap, c.tracker_status, c.k_status), name
    finally:
        ctx.set_param("tracker_scan_ladder_max_ks", ROUTES["default"])


def test_timed_mode_gives_the_same_words(env, cs):
    N, ctx = env
    c = cs["differential 16 x 130"]
    ctx.set_param("tracker_scan_timing", 1)
    try:
        assert native_match(N, c, ctx, tile=5) == (c.bitmap, c.tracker_status, c.k_status)
        ms = (ctypes.c_float * 2)()
        assert N.cg1_tracker_match_last_ms(ctx.handle, ms) == N.OK and ms[0] > 0 and ms[1] > 0
    finally:
        ctx.set_param("tracker_scan_timing", 0)
    assert native_match(N, c, ctx) == (c.bitmap, c.tracker_status, c.k_status)
    assert N.cg1_tracker_match_last_ms(ctx.handle, ms) == N.OK and ms[0] == 0 and ms[1] == 0


def test_refusals_write_nothing(env, cs):
    N, ctx = env
    c = cs["3 x 65"]
    T, V = len(c.trackers), len(c.ks)
    bm = ctypes.create_string_buffer(b"\xa5" * (16 * T), 16 * T)
    ts, ks = (ctypes.c_int32 * T)(*([-1] * T)), (ctypes.c_int32 * V)(*([-1] * V))
    for args in ((None, T, c.ks32, V, 0, bm, ts, ks), (c.trackers96, T, None, V, 0, bm, ts, ks), (c.trackers96, T, c.ks32, V, 0, None, ts, ks),
                 (c.trackers96, T, c.ks32, V, 0, bm, None, ks), (c.trackers96, T, c.ks32, V, 0, bm, ts, None), (c.trackers96, T, c.ks32, V, 4097, bm, ts, ks),
                 (c.trackers96, 65537, c.ks32, V, 0, bm, ts, ks), (c.trackers96, T, c.ks32, (1 << 20) + 1, 0, bm, ts, ks),
                 (c.trackers96, 65536, c.ks32, 1 << 20, 0, bm, ts, ks)):
        assert N.cg1_tracker_match_device(ctx.handle, *args) == N.ERR_ARG
        assert bm.raw == b"\xa5" * (16 * T) and list(ts) == [-1] * T and list(ks) == [-1] * V
        text = N.cg1_ctx_error(ctx.handle).decode()
        assert text.startswith("cg1_tracker_match_device") and c.ks32[:8].hex() not in text
    assert N.cg1_tracker_match_device(ctx.handle, None, 0, None, 0, 0, None, None, None) == N.OK
    assert N.cg1_tracker_match_device(ctx.handle, None, 0, c.ks32, V, 0, None, None, ks) == N.OK and list(ks) == c.k_status
    assert N.cg1_tracker_match_device(ctx.handle, c.trackers96, T, None, 0, 0, None, ts, None) == N.OK and list(ts) == c.tracker_status


def test_python_face_on_the_device(env, cs):
    from curdleproofs_pie_amd.tracker_scan import TrackerScanner, find_matching_trackers, is_matching_tracker

    N, ctx = env
    for name in ("2 x 130", "scalars and identities", "bad encodings"):
        c = cs[name]
        sc = TrackerScanner(ctx, device=True)
        assert sc.scan(c.trackers, c.ks) == pairs_of(c)
        assert sc.last_tracker_status == c.tracker_status and sc.last_k_status == c.k_status
        assert sc.scan_packed(c.trackers96, c.ks32) == (c.bitmap, c.tracker_status, c.k_status)
    c = cs["differential 16 x 130"]
    assert TrackerScanner(ctx, device=True, max_trackers=3, max_ks=7, tile_bases=2).scan_packed(c.trackers96, c.ks32) == (c.bitmap, c.tracker_status, c.k_status)
    assert find_matching_trackers(c.trackers, c.ks, ctx=ctx, device=True) == pairs_of(c)
    n = cs["near misses"]
    assert is_matching_tracker(n.trackers[0], n.ks[0], ctx=ctx, device=True) is True
    assert is_matching_tracker(n.trackers[1], n.ks[0], ctx=ctx, device=True) is False
    b = cs["bad encodings"]
    assert is_matching_tracker(b.trackers[1], b.ks[0], ctx=ctx, device=True) is False
    # device=None: this many pairs go to the GPU, and give the same pairs as the host twin
    sc = TrackerScanner(ctx)
    sc.HOST_MAX_PAIRS = 100
    assert sc._on_device(16 * 130) and sc.scan(c.trackers, c.ks) == TrackerScanner(device=False).scan(c.trackers, c.ks)
