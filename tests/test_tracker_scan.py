"""The tracker scan on the host: cg1_tracker_match (decode, multiply, compare on the worker pool) and the Python face over it against
the oracle's matrices (tests/tracker_scan_cases.py) -- every word of every bitmap, padding bits included, and every status.  No GPU:
tests/test_tracker_scan_gpu.py asks the same of the device and holds it against this twin bit for bit."""
import ctypes

import pytest

import tracker_scan_cases as S
from oracle import bls12_381 as O

NAMES = ["1 x 1", "3 x 65", "5 x 64, tile 2", "2 x 130", "near misses", "scalars and identities", "whole curve", "bad encodings", "reference vectors",
         "differential 16 x 130"]


@pytest.fixture(scope="module")
def cs():
    return S.cases()


def native_match(N, c, ctx=None, tile=None):
    """-> (bitmap bytes, tracker status, k status) of one native call, the buffers pre-filled so that an unwritten word shows."""
    T, V = len(c.trackers), len(c.ks)
    bm = ctypes.create_string_buffer(b"\xa5" * (8 * c.words * T), 8 * c.words * T)
    ts, ks = (ctypes.c_int32 * T)(*([-1] * T)), (ctypes.c_int32 * V)(*([-1] * V))
    tile = c.tile if tile is None else tile
    if ctx is None:
        rc = N.cg1_tracker_match(c.trackers96, T, c.ks32, V, tile, bm, ts, ks)
    else:
        rc = N.cg1_tracker_match_device(ctx.handle, c.trackers96, T, c.ks32, V, tile, bm, ts, ks)
    assert rc == N.OK
    return bm.raw, list(ts), list(ks)


def test_the_cases_are_what_they_say(cs):
    assert sorted(cs) == sorted(NAMES)
    assert S.light_digits(8) == [8] + [0] * 63 and S.light_digits(9)[:2] == [-7, 1] and S.light_digits(O.R - 1)[-1] in (7, 8)
    # order 3 (16^w = 1 mod 3): 3 is an identity entry met by an identity accumulator; 1 + 16 adds the entry to itself; 1 + 2 * 16 cancels and
    # 1 + 2 * 16 + 256 revives; 1 + 3 * 16 meets an identity entry with a finite accumulator
    assert S.window_events(3, 3) == ({S.EVENTS[3]}, 0) and S.window_events(3, 17) == ({S.EVENTS[0]}, 2)
    assert S.window_events(3, 33) == ({S.EVENTS[1]}, 0) and S.window_events(3, 289) == ({S.EVENTS[1], S.EVENTS[4]}, 1)
    assert S.window_events(3, 49) == ({S.EVENTS[2]}, 1)
    assert all(cs["whole curve"].events[e] > 0 for e in S.EVENTS)
    assert S.window_events(O.R, O.R - 1)[0] == set()                    # a prime-order base under a canonical scalar meets none of them
    shapes = {(len(c.trackers), len(c.ks), c.tile) for c in cs.values()}
    assert {(1, 1, 0), (3, 65, 0), (5, 64, 2), (2, 130, 0), (16, 130, 0)} <= shapes
    d = cs["scalars and identities"]
    assert d.bitmap[8 * 3: 8 * 4] == (0b100111).to_bytes(8, "little")   # the dense row: every live secret, not the refused ones


@pytest.mark.parametrize("name", NAMES)
def test_host_twin(native_lib, cs, name):
    c = cs[name]
    bitmap, ts, ks = native_match(native_lib, c)
    assert ts == c.tracker_status and ks == c.k_status
    assert bitmap == c.bitmap
    if c.tile:                                                          # the host twin has no tiles: the argument changes nothing
        assert native_match(native_lib, c, tile=0) == (bitmap, ts, ks)


def test_refusals_write_nothing(native_lib, cs):
    N, c = native_lib, cs["3 x 65"]
    T, V = len(c.trackers), len(c.ks)
    bm = ctypes.create_string_buffer(b"\xa5" * (16 * T), 16 * T)
    ts, ks = (ctypes.c_int32 * T)(*([-1] * T)), (ctypes.c_int32 * V)(*([-1] * V))
    for args in ((None, T, c.ks32, V, 0, bm, ts, ks), (c.trackers96, T, None, V, 0, bm, ts, ks), (c.trackers96, T, c.ks32, V, 0, None, ts, ks),
                 (c.trackers96, T, c.ks32, V, 0, bm, None, ks), (c.trackers96, T, c.ks32, V, 0, bm, ts, None), (c.trackers96, T, c.ks32, V, 4097, bm, ts, ks),
                 (c.trackers96, 65537, c.ks32, V, 0, bm, ts, ks), (c.trackers96, T, c.ks32, (1 << 20) + 1, 0, bm, ts, ks),
                 (c.trackers96, 65536, c.ks32, 1 << 20, 0, bm, ts, ks)):
        assert N.cg1_tracker_match(*args) == N.ERR_ARG
        assert bm.raw == b"\xa5" * (16 * T) and list(ts) == [-1] * T and list(ks) == [-1] * V
    assert N.cg1_tracker_match(None, 0, None, 0, 0, None, None, None) == N.OK
    assert N.cg1_tracker_match(None, 0, c.ks32, V, 0, None, None, ks) == N.OK and list(ks) == c.k_status
    assert N.cg1_tracker_match(c.trackers96, T, None, 0, 0, None, ts, None) == N.OK and list(ts) == c.tracker_status


# ------------------------------------------------------------------ the Python face (device=False: the host twin)
def pairs_of(c):
    return sorted((j, i) for i, j in c.bits)


def test_scan_returns_the_bitmaps_pairs(native_lib, cs):
    from curdleproofs_pie_amd.tracker_scan import TrackerScanner, find_matching_trackers

    for name in ("3 x 65", "scalars and identities", "bad encodings"):
        c = cs[name]
        sc = TrackerScanner(device=False)
        trackers, ks = list(c.trackers), list(c.ks)
        got = sc.scan(trackers, ks)
        assert got == pairs_of(c) and got == sorted(got)
        assert sc.last_tracker_status == c.tracker_status and sc.last_k_status == c.k_status
        assert trackers == c.trackers and ks == c.ks                     # inputs are not mutated
        assert sc.scan_packed(c.trackers96, c.ks32) == (c.bitmap, c.tracker_status, c.k_status)
        assert find_matching_trackers(trackers, ks, device=False) == got

    class Tracker:
        def __init__(self, r, s):
            self.r_G, self.k_r_G = r, s

    c = cs["2 x 130"]
    ks = [k.to_bytes(32, "little") if j % 2 else k for j, k in enumerate(c.ks)]
    assert TrackerScanner(device=False).scan([Tracker(r, s) for r, s in c.trackers], ks) == pairs_of(c)


def test_is_matching_tracker(native_lib, cs):
    from curdleproofs_pie_amd.tracker_scan import is_matching_tracker

    c = cs["near misses"]
    assert is_matching_tracker(c.trackers[0], c.ks[0], device=False) is True
    assert all(is_matching_tracker(t, c.ks[0], device=False) is False for t in c.trackers[1:])
    b = cs["bad encodings"]
    assert b.tracker_status[1] == S.BAD_POINT and is_matching_tracker(b.trackers[1], b.ks[0], device=False) is False
    assert is_matching_tracker(b.trackers[0], b.ks[0], device=False) is True
    assert is_matching_tracker(c.trackers[0], O.R, device=False) is False            # no Scalar
    assert is_matching_tracker(c.trackers[0], -1, device=False) is False
    assert is_matching_tracker((c.trackers[0][0][:47], c.trackers[0][1]), c.ks[0], device=False) is False


def test_shape_and_type_errors_come_before_any_native_call(native_lib, cs, monkeypatch):
    from curdleproofs_pie_amd import tracker_scan as TS

    def boom(*a):
        raise AssertionError("a native call was made")

    monkeypatch.setattr(TS.N, "cg1_tracker_match", boom)
    monkeypatch.setattr(TS.N, "cg1_tracker_match_device", boom)
    c = cs["1 x 1"]
    sc = TS.TrackerScanner(device=False)
    r, s = c.trackers[0]
    for trackers, ks, exc in (([(r[:47], s)], c.ks, ValueError), ([(r, s + b"\0")], c.ks, ValueError), ([(r,)], c.ks, ValueError), ([(r, 5)], c.ks, TypeError),
                              ([(r, s)], [1 << 256], ValueError), ([(r, s)], [-1], ValueError), ([(r, s)], [b"\1" * 31], ValueError), ([(r, s)], [None], TypeError)):
        with pytest.raises(exc):
            sc.scan(trackers, ks)
    for t96, k32, exc in ((c.trackers96[:-1], c.ks32, ValueError), (c.trackers96, c.ks32 + b"\0", ValueError), ("x" * 96, c.ks32, TypeError), (c.trackers96, 7, TypeError)):
        with pytest.raises(exc):
            sc.scan_packed(t96, k32)
    with pytest.raises(ValueError):
        TS.TrackerScanner(max_ks=0)
    # the empty cases make no native call either
    assert sc.scan([], []) == [] and sc.scan_packed(b"", b"") == (b"", [], [])
    assert sc.last_tracker_status == [] and sc.last_k_status == []


def test_empty_sides(native_lib, cs):
    from curdleproofs_pie_amd.tracker_scan import TrackerScanner

    c = cs["bad encodings"]
    sc = TrackerScanner(device=False)
    assert sc.scan(c.trackers, []) == [] and sc.last_tracker_status == c.tracker_status and sc.last_k_status == []
    d = cs["scalars and identities"]
    assert sc.scan([], d.ks) == [] and sc.last_k_status == d.k_status and sc.last_tracker_status == []


@pytest.mark.parametrize("max_trackers,max_ks", [(2, 1 << 20), (65536, 64), (3, 7), (1, 1)])
def test_chunked_equals_unchunked(native_lib, cs, max_trackers, max_ks):
    from curdleproofs_pie_amd.tracker_scan import TrackerScanner

    c = cs["5 x 64, tile 2"] if (max_trackers, max_ks) == (1, 1) else cs["differential 16 x 130"]
    sc = TrackerScanner(device=False, max_trackers=max_trackers, max_ks=max_ks)
    assert sc.scan_packed(c.trackers96, c.ks32) == (c.bitmap, c.tracker_status, c.k_status)
    b = cs["scalars and identities"]                                     # statuses of both kinds through the chunk seams
    assert sc.scan_packed(b.trackers96, b.ks32) == (b.bitmap, b.tracker_status, b.k_status)


def test_device_is_chosen_by_size_and_fails_loudly_without_one(native_lib, cs):
    from curdleproofs_pie_amd.tracker_scan import TrackerScanner

    sc = TrackerScanner()
    assert not sc._on_device(sc.HOST_MAX_PAIRS) and sc._on_device(sc.HOST_MAX_PAIRS + 1)
    assert TrackerScanner(device=True)._on_device(1) and not TrackerScanner(device=False)._on_device(1 << 30)
    if native_lib.cg1_device_count() == 0:
        c = cs["1 x 1"]
        with pytest.raises(native_lib.NativeError):
            TrackerScanner(device=True).scan(c.trackers, c.ks)
