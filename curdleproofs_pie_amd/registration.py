"""Whisk REGISTRATIONS made in bulk: per secret k the tracker, the k_commitment and the opening proof -- the reference's
generate_tracker(k) and get_k_commitment(k) (test_curdleproofs.py:759-790) and GenerateWhiskTrackerProof(tracker, k)
(whisk_interface.py:177-190 -> opening.py:33-56) for many validators at once.

Per item, with the two draws r (the tracker's) and b (the proof's blinder):

    r_G = r G    k_r_G = (k r mod FR_MODULUS) G    k_G = k G    A = b G    B = (b r mod FR_MODULUS) G

then the "whisk_opening_proof" transcript over [k_G, G, k_r_G, r_G, A, B], its challenge c and s = b - c k.  The tracker is r_G | k_r_G
(96 bytes), the k_commitment k_G (48), the proof A | B | s (128).  The maker knows r, so all five points are multiples of the generator:
batches take them from the GPU's table of G (cg1_whisk_register_device: csrc/kernels_register.h, one inversion per item above 32 768
items), up to 128 items run on the host's worker pool (cg1_whisk_register), byte for byte the same.
"""
from __future__ import annotations

import ctypes
import hashlib
import random
import secrets
from typing import List, Optional, Tuple

from . import _native as N
from .opening_prover import BAD_BLINDER, BAD_SCALAR, _scalar32      # status codes: 1 = k >= r, 4 = an r or b that is zero or >= r
from .shuffle_verifier import FR_MODULUS

DRAW_DOMAIN = b"whisk_registration_draw"
TRACKER_BYTES, COMMITMENT_BYTES, PROOF_BYTES = 96, 48, 128
MAX_ITEMS = (1 << 26) - 1                 # the per-call cap of the native entry points (include/curdle_g1.h: n < CG1_WHISK_REGISTER_MAX_ITEMS)


def registration_draws_from_seed(seed: bytes, index: int) -> Tuple[int, int]:
    """(r, b) of the registration with global index `index` under `seed` -- the format's definition:
    block(index, d) = SHAKE256(b"whisk_registration_draw" || seed || le64(index) || le32(d)).digest(64); r = int.from_bytes(block(index, 0),
    "little") % FR_MODULUS, b the same with d = 1.  What cg1_whisk_register_device derives on the device and cg1_whisk_register_draws on the host."""
    if len(seed) != 32:
        raise ValueError("seed: 32 bytes")
    if not 0 <= index < 1 << 32:
        raise ValueError("index: 0 .. 2^32 - 1")
    r, b = (int.from_bytes(hashlib.shake_256(DRAW_DOMAIN + seed + index.to_bytes(8, "little") + d.to_bytes(4, "little")).digest(64), "little") % FR_MODULUS
            for d in (0, 1))
    return r, b


class RegistrationBatchMaker:
    """Many (generate_tracker(k), get_k_commitment(k), GenerateWhiskTrackerProof(tracker, k)) triples as one batch.

    device=None: the host twin up to SMALL_HOST items, the GPU beyond; True / False force one side.  One maker = one caller at a time
    (`last_status` is per-object state).  max_items: the largest chunk handed to one native call (the native cap by default; tests force
    it small)."""

    # The host twin takes 4 - 5 us per item over its threads and the shortest device call ~1.0 ms of dependent launches: 0.66 against
    # 1.02 ms at 128 items, 1.17 against 1.08 ms at 256 (profiles/r22_registration_timing.txt).
    SMALL_HOST = 128

    def __init__(self, ctx: Optional["N.Context"] = None, device: Optional[bool] = None, max_items: int = MAX_ITEMS):
        if not 1 <= max_items <= MAX_ITEMS:
            raise ValueError("max_items: 1 .. %d" % MAX_ITEMS)
        self._ctx = ctx
        self.device = device
        self.max_items = int(max_items)
        self.last_status: List[int] = []

    @property
    def ctx(self) -> "N.Context":
        if self._ctx is None:
            self._ctx = N.default_context()
        return self._ctx

    def _on_device(self, n: int) -> bool:
        return n > self.SMALL_HOST if self.device is None else bool(self.device)

    def _call(self, on_device: bool, n: int, ks32: bytes, rs32: Optional[bytes], bl32: Optional[bytes], seed: Optional[bytes], first_index: int):
        trk = ctypes.create_string_buffer(TRACKER_BYTES * n)
        kcs = ctypes.create_string_buffer(COMMITMENT_BYTES * n)
        pfs = ctypes.create_string_buffer(PROOF_BYTES * n)
        st = (ctypes.c_int32 * n)()
        if on_device:
            ctx = self.ctx
            ctx.check(N.cg1_whisk_register_device(ctx.handle, n, ks32, rs32, bl32, seed if rs32 is None else None, first_index, trk, kcs, pfs, st))
        else:
            staged = None
            if rs32 is None:                               # the host twin takes supplied draws: derive them with the host's copy, wipe them after
                staged = (ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32 * n))
                rc = N.cg1_whisk_register_draws(seed, first_index, n, staged[0], staged[1])
                if rc:
                    raise N.NativeError(f"cg1_whisk_register_draws failed ({rc})")
                rs32, bl32 = staged
            try:
                rc = N.cg1_whisk_register(n, ks32, rs32, bl32, trk, kcs, pfs, st)
            finally:
                if staged is not None:
                    for b in staged:
                        ctypes.memset(b, 0, 32 * n)
            if rc:
                raise N.NativeError(f"cg1_whisk_register failed ({rc})")            # (never the inputs: they are secrets)
        return trk.raw, kcs.raw, pfs.raw, list(st)

    def make_packed(self, ks32: bytes, rs32: Optional[bytes] = None, blinders32: Optional[bytes] = None, seed: Optional[bytes] = None, first_index: int = 0):
        """n x k (and n x r, n x b, or neither) laid out back to back -> (n x 96 tracker bytes, n x 48 k_commitment bytes, n x 128 proof
        bytes, status per item).  Never touches `random`.  Without r and b, the draws of item i come from `seed` and the global index
        first_index + i (registration_draws_from_seed), so an item's bytes depend on (k, seed, index) alone and not on how a batch is cut;
        seed=None draws 32 fresh bytes from the OS per call.  A seed that is reused, or known to anyone but the maker, reveals every k it
        registered (k = (b - s) / c with b recomputed from the seed): pass one only in tests.  Status 0: made; 1: k >= FR_MODULUS; 4: an r or b,
        supplied or derived, that is zero or >= FR_MODULUS.  A refused item gets zero bytes in all three outputs.  k = 0 is legal."""
        for name, b in (("ks32", ks32), ("rs32", rs32), ("blinders32", blinders32)):
            if b is not None and not isinstance(b, (bytes, bytearray, memoryview)):
                raise TypeError(f"make_packed: {name} must be bytes")
        n = len(ks32) // 32
        if len(ks32) != 32 * n:
            raise ValueError("make_packed: ks32 must be n x 32 bytes")
        if (rs32 is None) != (blinders32 is None):
            raise ValueError("make_packed: rs32 and blinders32 are both given or both None")
        if rs32 is not None and (len(rs32) != 32 * n or len(blinders32) != 32 * n):
            raise ValueError("make_packed: expected n x 32 bytes of r and of b")
        if rs32 is None and seed is None:
            seed = secrets.token_bytes(32)
        if seed is not None and len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        if not 0 <= first_index or first_index + n > 1 << 32:
            raise ValueError("first_index + n must not pass 2^32")
        if n == 0:
            self.last_status = []
            return b"", b"", b"", []
        on_device = self._on_device(n)
        ks32 = bytes(ks32)
        rs32 = None if rs32 is None else bytes(rs32)
        blinders32 = None if blinders32 is None else bytes(blinders32)
        parts = []
        for lo in range(0, n, self.max_items):
            m = min(self.max_items, n - lo)
            cut = slice(32 * lo, 32 * (lo + m))
            parts.append(self._call(on_device, m, ks32[cut], None if rs32 is None else rs32[cut], None if blinders32 is None else blinders32[cut], seed,
                                    first_index + lo))
        trk, kcs, pfs = (b"".join(p[j] for p in parts) for j in range(3))
        status = [s for p in parts for s in p[3]]
        self.last_status = status
        return trk, kcs, pfs, status

    def make_many(self, ks, rng=None):
        """[(generate_tracker(k), get_k_commitment(k), GenerateWhiskTrackerProof(tracker, k)) for k in ks] as ((r_G, k_r_G), k_commitment,
        proof) byte strings, None for an item that is refused (its code in `last_status`).  Per item with k < FR_MODULUS, in input order,
        r = randint(1, FR_MODULUS - 1) is drawn and then b likewise, from the global `random` (or `rng`): exactly the reference's draws
        per validator, so under one random.seed the bytes equal the reference's and `random` ends in the same state."""
        ks32 = [_scalar32(k) for k in ks]
        n = len(ks32)
        draw = rng.randint if rng is not None else random.randint
        rs, bs = bytearray(32 * n), bytearray(32 * n)
        for i, k in enumerate(ks32):
            if int.from_bytes(k, "little") < FR_MODULUS:
                rs[32 * i: 32 * i + 32] = draw(1, FR_MODULUS - 1).to_bytes(32, "little")
                bs[32 * i: 32 * i + 32] = draw(1, FR_MODULUS - 1).to_bytes(32, "little")
        try:
            trk, kcs, pfs, status = self.make_packed(b"".join(ks32), bytes(rs), bytes(bs))
        finally:
            rs[:] = bytes(32 * n)                          # the staging of the draws is wiped (the immutable copies handed down are the interpreter's)
            bs[:] = bytes(32 * n)
        return [((trk[96 * i: 96 * i + 48], trk[96 * i + 48: 96 * i + 96]), kcs[48 * i: 48 * i + 48], pfs[128 * i: 128 * i + 128]) if s == 0 else None
                for i, s in enumerate(status)]


def make_whisk_registration(k, ctx=None):
    """((r_G, k_r_G), k_commitment, proof) for one secret k, with r and b derived from a fresh seed from the OS; raises ValueError where
    the reference would (k >= FR_MODULUS)."""
    out = make_whisk_registrations([k], ctx)[0]
    if out is None:
        raise ValueError("registration: k refused (not below FR_MODULUS)")
    return out


def make_whisk_registrations(ks, ctx=None, device: Optional[bool] = None):
    """[((r_G, k_r_G), k_commitment, proof) or None] for the secrets ks in one batch; the draws come from a fresh seed from the OS."""
    ks32 = b"".join(_scalar32(k) for k in ks)
    trk, kcs, pfs, status = RegistrationBatchMaker(ctx, device).make_packed(ks32)
    return [((trk[96 * i: 96 * i + 48], trk[96 * i + 48: 96 * i + 96]), kcs[48 * i: 48 * i + 48], pfs[128 * i: 128 * i + 128]) if s == 0 else None
            for i, s in enumerate(status)]
