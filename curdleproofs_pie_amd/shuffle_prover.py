"""Whisk shuffle proofs GENERATED in batches from tracker bytes: GenerateWhiskShuffleProof (whisk_interface.py:111-140) for many lists of
pre-shuffle trackers of one ell at once -- the counterpart of shuffle_verifier.ShuffleBatchVerifier.

Per item the reference decodes 2 ell points, multiplies them by k, permutes them, commits to the permutation (M), proves the shuffle
(CurdleProofsProof.new) and re-encodes 2 ell points.  Here all of it is ONE native call per batch (cg1_whisk_shuffle_prove_device:
csrc/capi_whisk_shuffle.h, csrc/kernels_whisk_shuffle.h, then the chain of csrc/capi_shuffle.h): tracker bytes in, post-shuffle tracker
bytes and M || proof out, no G1Point object on the way.

    prover = ShuffleBatchProver(crs)                         # crs: vec_G, vec_H, H, G_t, G_u
    out = prover.generate([pre_trackers_a, pre_trackers_b])  # [(post_trackers, whisk_shuffle_proof_bytes), ...]
    ShuffleBatchVerifier(crs_bytes).verify_many([(pre, post, proof) for pre, (post, proof) in zip(lists, out)])

One difference from the reference: a tracker point outside the prime-order subgroup G1 is refused (NativeError).  The reference decodes
trackers unchecked (util.py:35-36) and would go on; the device prover folds k into the scalars of its same-scalar block, which is exact
only for points of order r, so the call certifies every tracker point first.

generate() draws from Python's `random`, as the reference does: that is what the byte-for-byte tests need, and nothing to prove with.
To prove, use the seeded face: tracker bytes and a 32-byte seed in, every draw made on the device (cg1_whisk_shuffle_prove_seeded), a
status per shuffle out -- one malformed tracker costs its own list its proof and no other.

    post96, proofs, status = prover.generate_packed(trackers96)          # flat bytes; the seed: 32 fresh bytes from the OS, kept nowhere
    out = prover.generate_seeded(lists)                                   # [(post_trackers, proof) or None, ...]

shuffle_draws_from_seed is the definition of what a seed draws.
"""
from __future__ import annotations

import hashlib
import random
import secrets
from typing import List, Optional, Sequence, Tuple

from . import _native as N
from .opening_prover import _scalar32, _tracker_bytes
from .shuffle_verifier import FR_MODULUS

N_BLINDERS = 4                                                          # curdleproofs.py:24
DRAW_DOMAIN = b"whisk_shuffle_draw"
REJECT_NAMES = {0: "proved", N.WHISK_SHUFFLE_NO_DECODE: "a tracker point does not decode", N.WHISK_SHUFFLE_NOT_G1: "a tracker point outside G1"}
HALF_NAMES = ("r_G", "k_r_G")


def shuffle_draws_from_seed(seed: bytes, index: int, ell: int) -> tuple:
    """What shuffle number `index` of `seed` draws -> (permutation, k, vec_m_blinders, draws), the last four fields of a prove_many item:
    prove_many([(pre, *shuffle_draws_from_seed(seed, i, ell))]) is the definition of item i of generate_packed(.., seed).  Draw number d is
    block(d) = SHAKE256(b"whisk_shuffle_draw" || seed || le64(index) || le32(d)).digest(64); d = 0 .. ell - 2 are the Fisher-Yates steps
    i = ell - 1 - d, j = le128(block[:16]) mod (i + 1), swap perm[i], perm[j]; then one draw each for k, vec_m_blinders (4), vec_a_blinders (2),
    vec_c_blinders (4), ipa_r (n), ipa_z_head (n - 2), r_t, r_u, r_a, r_b, r_k and vec_r (n), n = ell + 4: le512(block) mod r, as 32-byte
    strings."""
    if len(seed) != 32:
        raise ValueError("seed: 32 bytes")
    if not 0 <= index < 1 << 32:
        raise ValueError("index: 0 .. 2^32 - 1")
    n = ell + N_BLINDERS
    head = DRAW_DOMAIN + bytes(seed) + index.to_bytes(8, "little")
    block = lambda d: hashlib.shake_256(head + d.to_bytes(4, "little")).digest(64)
    perm = list(range(ell))
    for d in range(ell - 1):
        i = ell - 1 - d
        j = int.from_bytes(block(d)[:16], "little") % (i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    count = iter(range(ell - 1, ell + 3 * n + 13))
    take = lambda m: [(int.from_bytes(block(next(count)), "little") % FR_MODULUS).to_bytes(32, "little") for _ in range(m)]
    k, mbl = take(1)[0], take(N_BLINDERS)
    abl, cbl, ipa_r, z_head = take(N_BLINDERS - 2), take(N_BLINDERS), take(n), take(n - 2)
    r_t, r_u, r_a, r_b, r_k = take(5)
    return perm, k, mbl, (abl, cbl, ipa_r, z_head, r_t, r_u, r_a, r_b, r_k, take(n))


def _draw_scalars(randint, m: int) -> List[bytes]:
    return [randint(1, FR_MODULUS - 1).to_bytes(32, "little") for _ in range(m)]


def _shuffle_draws(randint, ell: int) -> tuple:
    """prover_kernels.shuffle_draws with the caller's randint, as 32-byte strings: the draws of one CurdleProofsProof.new in the reference's order."""
    n = ell + N_BLINDERS
    vec_a_blinders, vec_c_blinders, ipa_r, ipa_z_head = (_draw_scalars(randint, m) for m in (N_BLINDERS - 2, N_BLINDERS, n, n - 2))
    r_t, r_u, r_a, r_b, r_k = _draw_scalars(randint, 5)
    return (vec_a_blinders, vec_c_blinders, ipa_r, ipa_z_head, r_t, r_u, r_a, r_b, r_k, _draw_scalars(randint, n))


class ShuffleBatchProver:
    """Many `GenerateWhiskShuffleProof(crs, pre_shuffle_trackers)` calls (whisk_interface.py:111-140) over one CRS as one batch.

    crs: any object with vec_G (ell points), vec_H (4), H, G_t and G_u as G1Points; ell + 4 is a power of two in 8 .. 1024.
    table: a fixed_base.FixedBaseTable holding those very objects (FixedBaseTable.for_crs(crs)); made here when not given, and then
    owned and closed by this prover (close(), or the `with` statement).
    resident_witness: the seeded calls (generate_packed, generate_seeded) keep what they draw on the device -- the context parameter
    "whisk_resident_witness", set around each native call and left at 0; the same bytes come out.  prove_many and generate() take the
    caller's draws, host data by definition, and do not look at it."""

    def __init__(self, crs, table=None, resident_witness=False):
        from .fixed_base import FixedBaseTable

        self.crs = crs
        self.ell = len(crs.vec_G)
        n = self.ell + N_BLINDERS
        if len(crs.vec_H) != N_BLINDERS or self.ell < 1 or n & (n - 1) or n < 8 or n > N.SAME_MSM_MAX_N:
            raise ValueError(f"a shuffle proof has 4 blinders and ell + 4 a power of two in 8 .. {N.SAME_MSM_MAX_N}, not ell = {self.ell} and {len(crs.vec_H)} blinders")
        self._owns = table is None
        if table is None:
            table = FixedBaseTable.for_crs(crs) if hasattr(crs, "G_sum") and hasattr(crs, "H_sum") else FixedBaseTable(
                list(crs.vec_G) + list(crs.vec_H) + [crs.H, crs.G_t, crs.G_u])
        self.table = table
        self.resident_witness = bool(resident_witness)
        self._fixed = None                                   # the table indices and G_t | G_u | H, looked up at the first call
        self.last_status: List[int] = []                     # of the last seeded call, per shuffle: a key of REJECT_NAMES
        self.last_refusals: List[Optional[Tuple[int, str]]] = []        # ... and (tracker index, "r_G" | "k_r_G") where the status is not 0

    def close(self) -> None:
        if self._owns and self.table is not None:
            self.table.close()
        self.table = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _crs_args(self):
        if self._fixed is None:
            from .py_arkworks_bls12381 import points_to_affine96

            t, crs = self.table, self.crs
            self._fixed = (list(t._indices(list(crs.vec_G), self.ell)), list(t._indices(list(crs.vec_H), N_BLINDERS)), t._indices([crs.H], 1)[0],
                           t._indices([crs.G_t], 1)[0], t._indices([crs.G_u], 1)[0], bytes(points_to_affine96([crs.G_t, crs.G_u, crs.H])))
        return self._fixed

    def _pack(self, items) -> list:
        """Every shape and type, before anything runs: -> per item (trackers96, perm, k32, mbl128, the six draw strings)."""
        ell, n = self.ell, self.ell + N_BLINDERS
        packed = []
        for it in items:
            it = tuple(it)
            if len(it) != 5:
                raise ValueError("an item is (pre_trackers, permutation, k, vec_m_blinders, draws)")
            pre, perm, k, mbl, draws = it
            pre, perm, mbl, draws = list(pre), list(perm), list(mbl), tuple(draws)
            if len(pre) != ell or len(perm) != ell or len(mbl) != N_BLINDERS:
                raise ValueError(f"pre_trackers and permutation have ell = {ell} entries, vec_m_blinders {N_BLINDERS}")
            if any(isinstance(m, bool) or not isinstance(m, int) for m in perm):
                raise TypeError("a permutation holds ints")
            if any(not 0 <= m < 1 << 32 for m in perm):
                raise ValueError("a permutation holds ints in 0 .. 2^32 - 1")
            trk = []
            for t in pre:
                r, kr = _tracker_bytes(t)
                if len(r) != 48 or len(kr) != 48:
                    raise ValueError("a tracker is two 48-byte encodings (r_G, k_r_G)")
                trk.append(r + kr)
            if len(draws) != 10:
                raise ValueError("draws are (vec_a_blinders (2), vec_c_blinders (4), ipa_r (n), ipa_z_head (n - 2), r_t, r_u, r_a, r_b, r_k, vec_r (n))")
            abl, cbl, ipa_r, z_head, vec_r = (list(draws[i]) for i in (0, 1, 2, 3, 9))
            if not (len(abl) == 2 and len(cbl) == N_BLINDERS and len(ipa_r) == n and len(z_head) == n - 2 and len(vec_r) == n):
                raise ValueError("draws are (vec_a_blinders (2), vec_c_blinders (4), ipa_r (n), ipa_z_head (n - 2), r_t, r_u, r_a, r_b, r_k, vec_r (n))")
            j = lambda v: b"".join(_scalar32(s) for s in v)
            packed.append((b"".join(trk), perm, _scalar32(k), j(mbl), j(abl), j(cbl), j(ipa_r), j(z_head), j(draws[4:9]), j(vec_r)))
        return packed

    def prove_many(self, items) -> List[Tuple[List[Tuple[bytes, bytes]], bytes]]:
        """items[p] = (pre_trackers, permutation, k, vec_m_blinders, draws): pre_trackers holds ell WhiskTracker-like objects (r_G, k_r_G) or
        byte pairs; permutation ell ints (not required to be a bijection); k and vec_m_blinders (4) Scalars, 32-byte strings or ints; draws as
        prover_kernels.shuffle_draws(ell) returns them.  -> per item (post_trackers, whisk_shuffle_proof_bytes): post_trackers a list of
        (r_G, k_r_G) byte pairs, the proof M || CurdleProofsProof.to_bytes() as the verifier takes it -- byte for byte what the reference's
        GenerateWhiskShuffleProof returns for those draws.  More items than one native call carries go as further calls.  No input is mutated.
        ValueError / TypeError: a shape or a type, before anything runs.  NativeError: a refusal of the native call (a scalar >= r, a
        tracker that does not decode, is off the curve or outside G1, a permutation entry >= ell, the divisions by zero of
        generate_ipa_blinders); nothing has been produced then."""
        packed = self._pack(list(items))
        if not packed:
            return []
        if self.table is None:
            raise N.NativeError("the prover is closed")
        ell, n = self.ell, self.ell + N_BLINDERS
        wb = int(N.cg1_whisk_shuffle_proof_bytes(ell))
        step = min(N.SAME_MSM_MAX_PROVERS, N.LIGHT_MAX_BASES // (2 * n))
        out = []
        table = self.table
        with table._ctx_lock():
            if table._KIND != "fixed-base":
                raise TypeError("the device pipeline of a shuffle proof runs over a FixedBaseTable")
            gi, hi, ui, gti, gui, gth = self._crs_args()
            for lo in range(0, len(packed), step):
                part = packed[lo: lo + step]
                P = len(part)
                col = lambda c: b"".join(pr[c] for pr in part)
                post, proofs = table._ctx.whisk_shuffle_prove_device(
                    table._tab, ell, P, gi * P, hi * P, [ui] * P, [gti] * P, [gui] * P, gth, col(0), [m for pr in part for m in pr[1]], col(2), col(3), col(4),
                    col(5), col(6), col(7), col(8), col(9))
                for p in range(P):
                    rec = post[96 * ell * p: 96 * ell * (p + 1)]
                    out.append(([(rec[96 * i: 96 * i + 48], rec[96 * i + 48: 96 * i + 96]) for i in range(ell)], proofs[wb * p: wb * (p + 1)]))
        return out

    def generate_packed(self, trackers96: bytes, seed: Optional[bytes] = None, first_index: int = 0) -> Tuple[bytes, bytes, List[int]]:
        """Shuffles proved from tracker bytes and a seed, flat buffers in and out, every draw made on the device.  trackers96: ell records
        r_G48 | k_r_G48 per shuffle.  -> (post96: ell records T48 | U48 per shuffle; proofs: cg1_whisk_shuffle_proof_bytes(ell) bytes M || proof
        per shuffle; status per shuffle, REJECT_NAMES).  Shuffle p draws what shuffle_draws_from_seed(seed, first_index + p, ell) gives, so its
        output depends on neither its neighbours nor on how the batch is cut into native calls.  A refused shuffle (status != 0: one of its
        tracker points does not decode or lies outside G1; `last_refusals` names the first) gets zero bytes in both outputs and leaves the
        others alone.  seed=None draws 32 fresh bytes from the OS and keeps them nowhere.  A seed that is reused, or known to anyone but the
        prover, reveals every k and permutation it proved: pass one only in tests.  Never touches `random`.
        ValueError: a length, before anything runs.  NativeError: a refusal of the whole native call; nothing has been produced then."""
        ell = self.ell
        trackers96 = bytes(trackers96)
        if len(trackers96) % (96 * ell):
            raise ValueError(f"trackers96: a multiple of 96 * ell = {96 * ell} bytes")
        count = len(trackers96) // (96 * ell)
        if seed is None:
            seed = secrets.token_bytes(32)
        seed = bytes(seed)
        if len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        if isinstance(first_index, bool) or not isinstance(first_index, int) or first_index < 0 or first_index + count > 1 << 32:
            raise ValueError("first_index: an int with first_index + the number of shuffles <= 2^32")
        self.last_status, self.last_refusals = [], []
        if not count:
            return b"", b"", []
        if self.table is None:
            raise N.NativeError("the prover is closed")
        step = min(N.SAME_MSM_MAX_PROVERS, N.LIGHT_MAX_BASES // (2 * (ell + N_BLINDERS)))
        posts, proofs, status, refusals = [], [], [], []
        table = self.table
        with table._ctx_lock():
            if table._KIND != "fixed-base":
                raise TypeError("the device pipeline of a shuffle proof runs over a FixedBaseTable")
            gi, hi, ui, gti, gui, gth = self._crs_args()
            table._ctx.set_param("whisk_resident_witness", int(self.resident_witness))
            try:
                for lo in range(0, count, step):
                    P = min(step, count - lo)
                    post, out, st, at = table._ctx.whisk_shuffle_prove_seeded(table._tab, ell, P, gi * P, hi * P, [ui] * P, [gti] * P, [gui] * P, gth,
                                                                              trackers96[96 * ell * lo: 96 * ell * (lo + P)], seed, first_index + lo)
                    posts.append(post); proofs.append(out); status += st
                    refusals += [(a >> 1, HALF_NAMES[a & 1]) if s else None for s, a in zip(st, at)]
            finally:
                table._ctx.set_param("whisk_resident_witness", 0)
        self.last_status, self.last_refusals = status, refusals
        return b"".join(posts), b"".join(proofs), list(status)

    def generate_seeded(self, pre_tracker_lists: Sequence, seed: Optional[bytes] = None, first_index: int = 0) -> List[Optional[Tuple[List[Tuple[bytes, bytes]], bytes]]]:
        """generate_packed over lists of ell WhiskTracker-like objects (r_G, k_r_G) or byte pairs: -> per list (post_trackers, proof) as
        prove_many returns them, or None where the list was refused (`last_status`, `last_refusals`).  No input is mutated."""
        ell = self.ell
        recs = []
        for pre in pre_tracker_lists:
            pre = list(pre)
            if len(pre) != ell:
                raise ValueError(f"pre_trackers has ell = {ell} entries")
            for t in pre:
                r, kr = _tracker_bytes(t)
                if len(r) != 48 or len(kr) != 48:
                    raise ValueError("a tracker is two 48-byte encodings (r_G, k_r_G)")
                recs.append(r + kr)
        post, proofs, status = self.generate_packed(b"".join(recs), seed, first_index)
        wb = len(proofs) // max(1, len(status))
        out = []
        for p, st in enumerate(status):
            rec = post[96 * ell * p: 96 * ell * (p + 1)]
            out.append(None if st else ([(rec[96 * i: 96 * i + 48], rec[96 * i + 48: 96 * i + 96]) for i in range(ell)], proofs[wb * p: wb * (p + 1)]))
        return out

    def generate(self, pre_tracker_lists: Sequence, rng: Optional[random.Random] = None) -> List[Tuple[List[Tuple[bytes, bytes]], bytes]]:
        """[GenerateWhiskShuffleProof(crs, pre) for pre in pre_tracker_lists] as one batch.  Per item, in the reference's order, it draws
        random.shuffle(list(range(ell))), k = random_scalar(), the four vec_m_blinders, then the draws of CurdleProofsProof.new
        (prover_kernels.shuffle_draws) -- from the global `random`, or from `rng` -- and then proves all items (prove_many).  After
        random.seed(s) the output equals the reference's for the same lists, called one after the other under the same seed, byte for byte,
        and `random` ends in the reference's state.  All draws are made before anything is proved: after a call that raises, the state of
        `random` (or `rng`) is unspecified -- the reference would have stopped drawing at the item that failed."""
        src = rng if rng is not None else random
        items = []
        for pre in pre_tracker_lists:
            perm = list(range(self.ell))
            src.shuffle(perm)
            k = _draw_scalars(src.randint, 1)[0]
            mbl = _draw_scalars(src.randint, N_BLINDERS)
            items.append((pre, perm, k, mbl, _shuffle_draws(src.randint, self.ell)))
        return self.prove_many(items)


def generate_whisk_shuffle_proof(crs, pre_trackers, table=None):
    """Drop-in for GenerateWhiskShuffleProof (whisk_interface.py:111-140) -- a batch of one -> (post_trackers as (r_G, k_r_G) byte pairs,
    whisk_shuffle_proof_bytes)."""
    return generate_whisk_shuffle_proofs(crs, [pre_trackers], table)[0]


def generate_whisk_shuffle_proofs(crs, lists, table=None):
    """[GenerateWhiskShuffleProof(crs, pre) for pre in lists] in one batch."""
    with ShuffleBatchProver(crs, table) as prover:
        return prover.generate(lists)
