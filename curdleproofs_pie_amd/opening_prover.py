"""Whisk tracker-opening proofs GENERATED in batches: GenerateWhiskTrackerProof (whisk_interface.py:177-190) ->
TrackerOpeningProof.new (opening.py:33-56) for many (tracker, k) at once, and fixed-base multiples of the generator.

Per item, in the reference's order: decode k_r_G and r_G unchecked (a bad encoding raises ValueError BEFORE a blinder is drawn),
k_G = k G, draw the blinder b, A = b G, B = b r_G, the transcript over [k_G, G, k_r_G, r_G, A, B] re-serialised and its challenge c,
s = b - c k; the proof is A | B | s (128 bytes) and k_G is the caller's k_commitment.  Large batches run on the GPU
(cg1_opening_prove_device: csrc/kernels_opening.h, csrc/kernels_generator.h), small ones on the host's worker pool
(cg1_opening_prove), byte for byte the same.
"""
from __future__ import annotations

import ctypes
import hashlib
import random
import secrets
from typing import List, Optional

from . import _native as N
from .shuffle_verifier import FR_MODULUS, REJECT_LENGTH

PROOF_BYTES = 128
BLINDER_DOMAIN = b"whisk_opening_blinder"
BAD_POINT, BAD_SCALAR, BAD_BLINDER = 2, 1, 4          # cg1_opening_prove's status codes (include/curdle_g1.h); REJECT_LENGTH = 5


def blinders_from_seed(seed: bytes, n: int, first: int = 0) -> bytes:
    """n x 32 bytes: b_i = int.from_bytes(SHAKE256(b"whisk_opening_blinder" || seed || le64(i)).digest(64), "little") mod r -- what
    cg1_opening_prove_device derives on the device when it gets no blinders."""
    if len(seed) != 32:
        raise ValueError("seed: 32 bytes")
    out = []
    for i in range(first, first + n):
        v = int.from_bytes(hashlib.shake_256(BLINDER_DOMAIN + seed + i.to_bytes(8, "little")).digest(64), "little") % FR_MODULUS
        out.append(v.to_bytes(32, "little"))
    return b"".join(out)


def _scalar32(k) -> bytes:
    """A Scalar (to_le_bytes), a 32-byte string or a non-negative int below 2^256, as 32 little-endian bytes (>= r is the native code's to reject)."""
    if hasattr(k, "to_le_bytes"):
        return bytes(k.to_le_bytes())
    if isinstance(k, (bytes, bytearray, memoryview)):
        b = bytes(k)
        if len(b) != 32:
            raise ValueError("scalar: 32 bytes")
        return b
    v = int(k)
    if not 0 <= v < 1 << 256:
        raise ValueError("scalar out of range")
    return v.to_bytes(32, "little")


def _tracker_bytes(t):
    r = t.r_G if hasattr(t, "r_G") else t[0]
    kr = t.k_r_G if hasattr(t, "k_r_G") else t[1]
    return bytes(r), bytes(kr)


class OpeningBatchProver:
    """Many `GenerateWhiskTrackerProof(tracker, k)` calls (whisk_interface.py:177-190) as one batch.

    device=None: the host twin up to SMALL_HOST items, the GPU beyond; True / False force one side.  One prover = one caller at a time
    (`last_status` is per-object state)."""

    PROOF_BYTES = PROOF_BYTES
    SMALL_HOST = 64                     # ~0.2 ms of scalar multiplications per proof over the pool's threads against ~2-3 ms of dependent launches

    def __init__(self, ctx: Optional["N.Context"] = None, device: Optional[bool] = None):
        self._ctx = ctx
        self.device = device
        self.last_status: List[int] = []

    @property
    def ctx(self) -> "N.Context":
        if self._ctx is None:
            self._ctx = N.default_context()
        return self._ctx

    def _on_device(self, n: int) -> bool:
        return n > self.SMALL_HOST if self.device is None else bool(self.device)

    def prove_packed(self, trackers96: bytes, ks32: bytes, blinders32: Optional[bytes] = None, seed: Optional[bytes] = None):
        """n proofs from n x (r_G | k_r_G), n x k and n x blinder (or none) laid out back to back -> (n x 128 proof bytes, n x 48 k_commitment
        bytes, status per item).  Never touches `random`.  Without blinders, blinder i is derived from `seed` (blinders_from_seed); seed=None
        draws 32 fresh bytes from the OS per call.  A seed that is reused, or known to anyone but the prover, reveals every k it proved
        (k = (b - s) / c with b recomputed from the seed): pass one only in tests.  A rejected item (status != 0) gets zero bytes."""
        n = len(ks32) // 32
        if len(ks32) != 32 * n or len(trackers96) != 96 * n or (blinders32 is not None and len(blinders32) != 32 * n):
            raise ValueError("prove_packed: expected n x 96, n x 32 (and n x 32) bytes")
        if blinders32 is None and seed is None:
            seed = secrets.token_bytes(32)
        if seed is not None and len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        if n == 0:
            self.last_status = []
            return b"", b"", []
        proofs = ctypes.create_string_buffer(128 * n)
        kcs = ctypes.create_string_buffer(48 * n)
        st = (ctypes.c_int32 * n)()
        if self._on_device(n):
            ctx = self.ctx
            ctx.check(N.cg1_opening_prove_device(ctx.handle, n, bytes(trackers96), bytes(ks32), None if blinders32 is None else bytes(blinders32),
                                                 seed if blinders32 is None else None, proofs, kcs, st))
        else:
            bl = bytes(blinders32) if blinders32 is not None else blinders_from_seed(seed, n)
            rc = N.cg1_opening_prove(n, bytes(trackers96), bytes(ks32), bl, proofs, kcs, st)
            if rc:
                raise N.NativeError(f"cg1_opening_prove failed ({rc})")
        status = [int(s) for s in st]
        self.last_status = status
        return proofs.raw, kcs.raw, status

    def _decodes(self, trackers96: bytes, n: int) -> List[bool]:
        """Which trackers decode (both points: from_compressed_bytes_unchecked raises otherwise, whisk_interface.py:182-183)."""
        if self._on_device(n):
            ctx = self.ctx
            d_in, d_aff, d_st = ctx.alloc(96 * n), ctx.alloc(192 * n), ctx.alloc(2 * n)
            try:
                d_in.upload(trackers96)
                ctx.check(N.cg1_batch_decompress_device(ctx.handle, d_in.ptr, d_aff.ptr, d_st.ptr, 2 * n, 0))
                st = d_st.download(2 * n)
            finally:
                for b in (d_in, d_aff, d_st):
                    b.free()
            return [st[2 * i] == 0 and st[2 * i + 1] == 0 for i in range(n)]
        inf = ctypes.c_int(0)
        return [N.cg1_validate_compressed(trackers96[96 * i + 48: 96 * i + 96], ctypes.byref(inf)) == N.OK
                and N.cg1_validate_compressed(trackers96[96 * i: 96 * i + 48], ctypes.byref(inf)) == N.OK for i in range(n)]

    def prove_many(self, items, blinders=None, rng=None) -> List[Optional[bytes]]:
        """[GenerateWhiskTrackerProof(tracker, k) for (tracker, k) in items], an item whose call would raise ValueError giving None (its code
        in `last_status`).  Items: (tracker, k) with a WhiskTracker-like tracker or an (r_G, k_r_G) byte pair and k a Scalar.  With no
        `blinders`, one randint(1, r - 1) is drawn per item that decodes, in input order, from the global `random` (or `rng`): exactly
        the reference's draws, so under one random.seed the proofs equal the reference's byte for byte and `random` ends in the same state."""
        items = list(items)
        n = len(items)
        trk, ks, pre = [], [], []
        for tracker, k in items:
            r, kr = _tracker_bytes(tracker)
            ok = len(r) == 48 and len(kr) == 48
            trk.append(r + kr if ok else bytes(96))
            ks.append(_scalar32(k))
            pre.append(0 if ok else REJECT_LENGTH)
        trackers96, ks32 = b"".join(trk), b"".join(ks)
        if blinders is None:
            draw = rng.randint if rng is not None else random.randint
            live = self._decodes(trackers96, n) if n else []
            bl = []
            for i in range(n):
                ok = live[i] and not pre[i] and int.from_bytes(ks[i], "little") < FR_MODULUS
                bl.append(draw(1, FR_MODULUS - 1).to_bytes(32, "little") if ok else bytes(32))
        else:
            bl = [_scalar32(b) for b in blinders]
            if len(bl) != n:
                raise ValueError("one blinder per item")
        proofs, kcs, status = self.prove_packed(trackers96, ks32, b"".join(bl))
        status = [p or s for p, s in zip(pre, status)]
        self.last_status = status
        self.last_k_commitments = [kcs[48 * i: 48 * i + 48] if s == 0 else None for i, s in enumerate(status)]
        return [proofs[128 * i: 128 * i + 128] if s == 0 else None for i, s in enumerate(status)]


def generate_whisk_tracker_proof(tracker, k, ctx=None) -> bytes:
    """Drop-in for GenerateWhiskTrackerProof (whisk_interface.py:177-190) -- a batch of one; raises ValueError where the reference does."""
    p = OpeningBatchProver(ctx)
    out = p.prove_many([(tracker, k)])[0]
    if out is None:
        raise ValueError(f"tracker proof: item rejected (code {p.last_status[0]})")
    return out


def generate_whisk_tracker_proofs(items, ctx=None) -> List[Optional[bytes]]:
    """[GenerateWhiskTrackerProof(tracker, k) for (tracker, k) in items] in one batch (None where the reference raises ValueError)."""
    return OpeningBatchProver(ctx).prove_many(items)


def generator_multiples(scalars, ctx=None, device: Optional[bool] = None) -> List[bytes]:
    """[bytes((G1 * k).to_compressed_bytes()) for k in scalars]: the Whisk k_commitment of each k.  Ints are taken mod r.  device=None:
    the host up to OpeningBatchProver.SMALL_HOST scalars, the GPU's fixed-base kernel (cg1_generator_mul_device) beyond."""
    sc = [(int(k) % FR_MODULUS).to_bytes(32, "little") if isinstance(k, int) else _scalar32(k) for k in scalars]
    n = len(sc)
    if n == 0:
        return []
    if n > OpeningBatchProver.SMALL_HOST if device is None else device:
        ctx = ctx or N.default_context()
        d_sc, d_out = ctx.alloc(32 * n), ctx.alloc(48 * n)
        try:
            d_sc.upload(b"".join(sc))
            ctx.check(N.cg1_generator_mul_device(ctx.handle, d_sc.ptr, n, None, d_out.ptr))
            raw = d_out.download(48 * n)
        finally:
            d_sc.free()
            d_out.free()
        return [raw[48 * i: 48 * i + 48] for i in range(n)]
    g = ctypes.create_string_buffer(N.POINT_BYTES)
    N.cg1_generator(g)
    tmp, out = ctypes.create_string_buffer(N.POINT_BYTES), ctypes.create_string_buffer(48)
    res = []
    for s in sc:
        N.cg1_mul(tmp, g.raw, s)
        N.cg1_compress(out, tmp.raw)
        res.append(out.raw)
    return res
