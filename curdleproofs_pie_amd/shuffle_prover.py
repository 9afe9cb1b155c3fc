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
"""
from __future__ import annotations

import random
from typing import List, Optional, Sequence, Tuple

from . import _native as N
from .opening_prover import _scalar32, _tracker_bytes
from .shuffle_verifier import FR_MODULUS

N_BLINDERS = 4                                                          # curdleproofs.py:24


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
    owned and closed by this prover (close(), or the `with` statement)."""

    def __init__(self, crs, table=None):
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
        self._fixed = None                                   # the table indices and G_t | G_u | H, looked up at the first call

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
