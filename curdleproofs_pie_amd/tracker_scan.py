"""Which trackers does a set of Whisk secrets open?  Before a validator can call GenerateWhiskTrackerProof it must know which tracker of the
list is its own: for each secret k and each tracker (r_G, k_r_G) it asks whether

    point_projective_from_bytes(r_G) * k == point_projective_from_bytes(k_r_G)        (util.py:35-36; the relation opening.py proves)

V secrets against T trackers are V * T scalar multiplications of variable bases.  Large scans run on the GPU (cg1_tracker_match_device,
csrc/kernels_tracker_scan.h: one light table per tracker serves every secret, 64 additions and no doubling per pair, no inversion; up to 32
secrets the same call runs one ladder per pair instead, which is cheaper there), small ones on the host's worker pool (cg1_tracker_match),
bit for bit the same.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple

from . import _native as N
from .opening_prover import BAD_POINT, BAD_SCALAR, _scalar32      # the status codes: 2 = a tracker point does not decode, 1 = k >= r

MAX_TRACKERS, MAX_KS, MAX_BITMAP_BYTES = 65536, 1 << 20, 1 << 30          # the per-call caps of the native entry points (include/curdle_g1.h)


def _tracker96(t) -> bytes:
    halves = (t.r_G, t.k_r_G) if hasattr(t, "r_G") else tuple(t)
    if len(halves) != 2:
        raise ValueError("tracker: (r_G, k_r_G)")
    for h in halves:
        if not isinstance(h, (bytes, bytearray, memoryview)):
            raise TypeError("tracker: r_G and k_r_G must be byte strings")
        if len(h) != 48:
            raise ValueError("tracker: r_G and k_r_G are 48 bytes each")
    return bytes(halves[0]) + bytes(halves[1])


class TrackerScanner:
    """`.scan(trackers, ks)` -> the sorted (k_index, tracker_index) pairs with ks[k_index] * r_G == k_r_G.

    device=None: the host twin up to HOST_MAX_PAIRS pairs, the GPU beyond; True / False force one side.  One scanner = one caller at a
    time (`last_tracker_status` / `last_k_status` are per-object state).  max_trackers / max_ks: the largest chunk handed to one native
    call (the native caps by default; tests force them small)."""

    # The host twin takes 5 - 7 us per pair over its threads (57 ms for 8 192 pairs, profiles/r16_tracker_scan_timing.txt) and the shortest
    # device call is a ladder's ~2.2 ms of dependent doublings whatever its size: they meet near 300 - 400 pairs.
    HOST_MAX_PAIRS = 256

    def __init__(self, ctx: Optional["N.Context"] = None, device: Optional[bool] = None, max_trackers: int = MAX_TRACKERS, max_ks: int = MAX_KS,
                 tile_bases: int = 0):
        if max_trackers < 1 or max_ks < 1 or max_trackers > MAX_TRACKERS or max_ks > MAX_KS:
            raise ValueError("max_trackers: 1 .. %d, max_ks: 1 .. %d" % (MAX_TRACKERS, MAX_KS))
        self._ctx = ctx
        self.device = device
        self.max_trackers, self.max_ks, self.tile_bases = int(max_trackers), int(max_ks), int(tile_bases)
        self.last_tracker_status: List[int] = []
        self.last_k_status: List[int] = []

    @property
    def ctx(self) -> "N.Context":
        if self._ctx is None:
            self._ctx = N.default_context()
        return self._ctx

    def _on_device(self, pairs: int) -> bool:
        return pairs > self.HOST_MAX_PAIRS if self.device is None else bool(self.device)

    def _call(self, on_device: bool, trackers96: bytes, T: int, ks32: bytes, V: int):
        words = (V + 63) // 64
        bm = ctypes.create_string_buffer(8 * words * T)
        ts, kst = (ctypes.c_int32 * T)(), (ctypes.c_int32 * V)()
        if on_device:
            ctx = self.ctx
            ctx.check(N.cg1_tracker_match_device(ctx.handle, trackers96, T, ks32, V, self.tile_bases, bm, ts, kst))
        else:
            rc = N.cg1_tracker_match(trackers96, T, ks32, V, self.tile_bases, bm, ts, kst)
            if rc:
                raise N.NativeError(f"cg1_tracker_match failed ({rc})")            # (never the inputs: they may be secrets)
        return bm.raw, list(ts), list(kst)

    def scan_packed(self, trackers96: bytes, ks32: bytes) -> Tuple[bytes, List[int], List[int]]:
        """T x (r_G | k_r_G) and V x k laid out back to back -> (bitmap, tracker status, k status).  bitmap: T x ceil(V / 64) little-endian
        64-bit words, word (i, j // 64) bit j % 64 = [k_j r_G_i == k_r_G_i]; a tracker with a point that does not decode (status 2) has
        a zero row, a secret >= r (status 1) a zero column.  Calls beyond the native caps are cut into chunks."""
        for name, b, unit in (("trackers96", trackers96, 96), ("ks32", ks32, 32)):
            if not isinstance(b, (bytes, bytearray, memoryview)):
                raise TypeError(f"scan_packed: {name} must be bytes")
            if len(b) % unit:
                raise ValueError(f"scan_packed: {name} must be a multiple of {unit} bytes")
        trackers96, ks32 = bytes(trackers96), bytes(ks32)
        T, V = len(trackers96) // 96, len(ks32) // 32
        words = (V + 63) // 64
        tstat, kstat = [0] * T, [0] * V
        if T == 0 or V == 0:
            if T or V:                                     # one side empty: the other side's statuses are still the native code's
                _, tstat, kstat = self._call(False if self.device is None else bool(self.device), trackers96, T, ks32, V)
            self.last_tracker_status, self.last_k_status = tstat, kstat
            return b"", tstat, kstat
        on_device = self._on_device(T * V)
        step_k = min(self.max_ks, V)
        step_t = max(1, min(self.max_trackers, T, MAX_BITMAP_BYTES // (8 * ((step_k + 63) // 64))))
        if step_t >= T and step_k >= V:
            bitmap, tstat, kstat = self._call(on_device, trackers96, T, ks32, V)
        else:
            rows = [0] * T                                 # a row as one integer: a chunk of secrets need not start at a word
            for t0 in range(0, T, step_t):
                nt = min(step_t, T - t0)
                for k0 in range(0, V, step_k):
                    nk = min(step_k, V - k0)
                    bm, ts, kst = self._call(on_device, trackers96[96 * t0: 96 * (t0 + nt)], nt, ks32[32 * k0: 32 * (k0 + nk)], nk)
                    w = (nk + 63) // 64
                    for i in range(nt):
                        rows[t0 + i] |= int.from_bytes(bm[8 * w * i: 8 * w * (i + 1)], "little") << k0
                    tstat[t0: t0 + nt] = ts
                    kstat[k0: k0 + nk] = kst
            bitmap = b"".join(r.to_bytes(8 * words, "little") for r in rows)
        self.last_tracker_status, self.last_k_status = tstat, kstat
        return bitmap, tstat, kstat

    def scan(self, trackers, ks) -> List[Tuple[int, int]]:
        """Sorted [(k_index, tracker_index)] over WhiskTracker-likes (or (r_G, k_r_G) byte pairs) and Scalars, ints or 32-byte strings.  A
        tracker half that is not 48 bytes raises ValueError (TypeError when it is no byte string), a k outside 0 .. 2^256 - 1 ValueError,
        before anything runs."""
        trk = [_tracker96(t) for t in trackers]
        ks32 = b"".join(_scalar32(k) for k in ks)
        bitmap, _, _ = self.scan_packed(b"".join(trk), ks32)
        T, V = len(trk), len(ks32) // 32
        words = (V + 63) // 64
        out = []
        for i in range(T if V else 0):
            row = int.from_bytes(bitmap[8 * words * i: 8 * words * (i + 1)], "little")
            while row:
                low = row & -row
                out.append((low.bit_length() - 1, i))
                row ^= low
        return sorted(out)


def find_matching_trackers(trackers, ks, ctx=None, device: Optional[bool] = None) -> List[Tuple[int, int]]:
    """[(k_index, tracker_index)], sorted: every pair with ks[k_index] * r_G == k_r_G."""
    return TrackerScanner(ctx, device).scan(trackers, ks)


def is_matching_tracker(tracker, k, ctx=None, device: Optional[bool] = None) -> bool:
    """point_projective_from_bytes(tracker.r_G) * k == point_projective_from_bytes(tracker.k_r_G) -- a scan of one pair; False where the
    reference expression would raise (an encoding that does not decode, a k that is no Scalar), as the IsValid* functions answer."""
    try:
        return TrackerScanner(ctx, device).scan([tracker], [k]) == [(0, 0)]
    except (ValueError, TypeError):
        return False
