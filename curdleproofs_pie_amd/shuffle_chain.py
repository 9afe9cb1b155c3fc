"""A chain of Whisk shuffles verified over a tracker set that stays on the device in decoded form.

Whisk produces its shuffles as a chain over ONE candidate set: N trackers (16 384 in the consensus spec); every block names `ell` slots of
it, proves a shuffle of what lies there and writes its post trackers back into the same slots.  After the first touch of a slot every pre
tracker of a block is the post tracker of an earlier block.  `ShuffleBatchVerifier` takes self-contained items (pre, post, proof) and decodes
all 4 ell + 89 points of each -- a square root per point, the verifier's dominant kernel -- although the 2 ell pre trackers were decoded
moments earlier as somebody's posts.  Here they are decoded once:

    TrackerSet            the N trackers as host bytes (authoritative) and as 2 N decoded records + status bytes on the device
    ShuffleChainVerifier  blocks as (indices, post trackers, proof) against a TrackerSet
    ShuffleChainProver    the other direction: ell slot indices per block and a seed in, such blocks out (its docstring; TrackerSet.evolve
                          is its tracker stage alone)

Semantics, block by block: block j reads pre_j = [set[i] for i in indices_j] BEFORE any of its own writes, then writes
set[indices_j[t]] = post_j[t] for t = 0 .. ell - 1 in order (indices of a block may repeat: the last write wins).  Its status is exactly
what `ShuffleBatchVerifier.verify_packed` returns for the expanded item (pre_j, post_j, proof_j) -- the codes of `REJECT_NAMES`; a post that
does not decode rejects its writer and then every reader of that slot, as it would there.  Every block is judged against the set as all
earlier blocks of the call left it, valid or not; on return the set holds the state after the longest prefix of blocks with status 0
(`last_stats["valid_prefix"]`).

How: `cg1_chain_expand` (native, one pass over the n 2 ell entries) expands the blocks to the verifier's instances -- the transcript hashes
every encoding -- and writes a source plan: where the decoded record of every pre position already is, an earlier block's post position in
the same batch or an entry of the resident set.  The one `ShuffleBatchVerifier` underneath (one pipeline, no coalescing) carries the plan in
its batch ticket: its decoding launch leaves the pre positions out (`k_batch_decompress_strided`), `k_chain_gather` copies their records in
behind it, `k_chain_scatter` writes the batch's final posts into the set behind the last sub-batch -- all on that verifier's one context
stream, in the order decode -> gather -> scatter -> next batch's decode, so batches rotate through its slots without further
synchronisation.  `last_stats["decoded_points"]` counts what was decoded: n (L - 2 ell), not n L.

Throughput against the expanded path (profiles/r20_chain_verify_timing.txt, tools/gpu_chain_verify_timing.py; DESIGN section 20 says what is
measured and what is not): at ell = 124 over 16 384 slots, 8 batches of 1 024 blocks, 4 hardware queues, the decoding launch takes 1.99 ms
instead of 3.35 per 1 024 blocks (2 ell / L = 42 %), but a chain runs on ONE pipeline -- its batches depend on each other through the set
-- and that pipeline is bound by its front-end launch: 7.9-8.2e4 blocks/s, no different from the expanded blocks on
ShuffleBatchVerifier(pipelines=1, coalesce=0) (8.0-8.1e4) and 0.6 x the default ShuffleBatchVerifier's 1.36-1.38e5.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

from . import _native as N
from .shuffle_verifier import REJECT_LENGTH, ShuffleBatchVerifier, _tracker_bytes
from .verifier_pipeline import Batch, sum_stats


_FR_MODULUS = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def _packed_trackers(trackers) -> bytes:
    """n x (r_G | k_r_G) from bytes of that form, WhiskTracker-likes or (r_G, k_r_G) pairs."""
    if isinstance(trackers, (bytes, bytearray, memoryview)):
        data = bytes(trackers)
        if len(data) % 96:
            raise ValueError("packed trackers: a multiple of 96 bytes")
        return data
    rs, ks = _tracker_bytes(trackers)
    return b"".join(rs[i: i + 48] + ks[i: i + 48] for i in range(0, len(rs), 48))


class TrackerSet:
    """N trackers: the host bytes (authoritative) and, on the device, their 2 N decoded records (r_G of slot s at point 2 s, k_r_G at
    2 s + 1; 96 bytes each, zeros for an encoding that does not decode) with the decoder's status bytes.  Belongs to one context; a
    ShuffleChainVerifier over it runs its device work on that context's stream.  One caller at a time."""

    def __init__(self, trackers, ctx: Optional["N.Context"] = None):
        self.ctx = ctx if ctx is not None else N.default_context()
        self.n_slots = 0
        self.d_wire = self.d_pts = self.d_pstat = None
        self._host = None
        self.replace(trackers)

    def __len__(self) -> int:
        return self.n_slots

    def packed(self) -> bytes:
        """The set as n_slots x (r_G | k_r_G) bytes."""
        return self._host.raw[: 96 * self.n_slots]

    def trackers(self) -> List[tuple]:
        """The set as (r_G, k_r_G) pairs of 48-byte encodings."""
        raw = self.packed()
        return [(raw[i: i + 48], raw[i + 48: i + 96]) for i in range(0, len(raw), 96)]

    def replace(self, trackers) -> None:
        """Another set (any size) in this one's place: new host bytes, one plain decoding launch over all of it."""
        data = _packed_trackers(trackers)
        n = len(data) // 96
        if n == 0:
            raise ValueError("an empty tracker set")
        if n != self.n_slots:
            self._free()
            self.d_wire, self.d_pts, self.d_pstat = self.ctx.alloc(96 * n), self.ctx.alloc(192 * n), self.ctx.alloc(2 * n)
            self.n_slots = n
        self._host = ctypes.create_string_buffer(data, len(data))
        self._load()

    def _load(self) -> None:
        """host bytes -> device records: the whole set"""
        ctx, n = self.ctx, self.n_slots
        self.d_wire.upload(self._host.raw[: 96 * n])
        ctx.check(N.cg1_batch_decompress_device(ctx.handle, self.d_wire.ptr, self.d_pts.ptr, self.d_pstat.ptr, 2 * n, 0))

    def _reload_slots(self, slots) -> None:
        """host bytes -> device records for `slots` only (distinct): their encodings decoded aside, then scattered into the set."""
        import numpy as np

        slots = np.asarray(slots, dtype=np.uint32)
        m = len(slots)
        if m == 0:
            return
        ctx = self.ctx
        raw = np.frombuffer(self._host, dtype=np.uint8, count=96 * self.n_slots).reshape(-1, 96)
        d_w, d_p, d_s = ctx.alloc(96 * m), ctx.alloc(192 * m), ctx.alloc(2 * m)
        try:
            d_w.upload(raw[slots].tobytes())
            ctx.check(N.cg1_batch_decompress_enqueue(ctx.handle, d_w.ptr, d_p.ptr, d_s.ptr, 2 * m, 0))
            pairs = np.empty((2 * m, 2), dtype="<u4")
            pairs[0::2, 0], pairs[1::2, 0] = 2 * slots, 2 * slots + 1
            pairs[:, 1] = np.arange(2 * m, dtype=np.uint32)
            ctx.check(N.cg1_chain_scatter_enqueue(ctx.handle, d_p.ptr, d_s.ptr, 2 * m, self.d_pts.ptr, self.d_pstat.ptr, 2 * self.n_slots, pairs.tobytes(), 2 * m))
            ctx.check(N.cg1_stream_sync(ctx.handle))
        finally:
            d_w.free(); d_p.free(); d_s.free()

    def _check_open(self) -> None:
        if self.d_pts is None or not self.ctx.handle:
            raise ValueError("the tracker set is closed")

    def _indices(self, indices, ell: int):
        """n x ell slot indices (ints, or uint32 little-endian bytes) -> (uint32 array, n); ValueError for an index outside the set or a count
        that is no multiple of ell"""
        import numpy as np

        if isinstance(indices, (bytes, bytearray, memoryview)):
            wide = np.frombuffer(bytes(indices), dtype="<u4").astype(np.int64)
        else:
            wide = np.asarray(indices, dtype=np.int64).reshape(-1)
        if len(wide) % ell:
            raise ValueError(f"{len(wide)} slot indices: not a multiple of ell = {ell}")
        if len(wide) and (wide.min() < 0 or wide.max() >= self.n_slots):
            raise ValueError(f"a slot index outside the set of {self.n_slots}")
        return np.ascontiguousarray(wide.astype("<u4")), len(wide) // ell

    def _apply_writers(self, writers, post96: bytes) -> None:
        """host bytes of every slot written <- the T | U record of its last writer (b ell + t names record b ell + t of post96)"""
        for slot, w in writers:
            ctypes.memmove(ctypes.addressof(self._host) + 96 * int(slot), post96[96 * int(w): 96 * int(w) + 96], 96)

    def _restore(self, before: bytes) -> None:
        """back to `before`, decoded afresh: what a failed call leaves (ShuffleChainVerifier.verify_blocks_packed's except branch)"""
        ctypes.memmove(self._host, before, len(before))
        try:
            self.ctx.check(N.cg1_stream_sync(self.ctx.handle))
            self._load()
        except Exception:
            pass

    def evolve(self, indices, perms, ks):
        """The tracker stage of a chain alone (cg1_chain_evolve_device), permutations and scalars the caller's: block j reads
        pre_j = [set[i] for i in indices_j] before any of its own writes and writes set[indices_j[t]] = ks[j] * pre_j[perms[j][t]], t in
        order.  indices: n lists of ell slots (ell: the length of perms[0]); perms: n permutations of 0 .. ell - 1; ks: n scalars (ints or
        32-byte little-endian strings, below r).  -> (post96, status): ell records T48 | U48 per block and a status per block, 0 or
        WHISK_SHUFFLE_NO_DECODE / WHISK_SHUFFLE_NOT_G1 for a block that read such a point -- it writes nothing, its records are zeros.
        The set is advanced, host bytes and device records.  `last_evolve_stats`: {"stage_ms", "certified_slots", "bad_at"}.  How a client
        that trusts a chain follows its trackers without verifying.  ValueError: a shape, an index, a permutation, k >= r -- before anything
        runs.  NativeError: the set is as it was before the call."""
        import numpy as np

        self._check_open()
        perms = [list(p) for p in perms]
        n = len(perms)
        ell = len(perms[0]) if n else 1
        if ell == 0 or any(len(p) != ell for p in perms):
            raise ValueError("perms: n permutations of one length ell >= 1")
        if any(sorted(p) != list(range(ell)) for p in perms):
            raise ValueError("perms: every row a permutation of 0 .. ell - 1")
        idx, n_idx = self._indices([i for block in indices for i in block] if not isinstance(indices, (bytes, bytearray, memoryview)) else indices, ell)
        ks = list(ks)
        if n_idx != n or len(ks) != n:
            raise ValueError("evolve: n x ell indices, n permutations and n scalars")
        k32 = bytearray()
        for k in ks:
            v = int.from_bytes(bytes(k), "little") if isinstance(k, (bytes, bytearray, memoryview)) else int(k)
            if not 0 <= v < _FR_MODULUS:
                raise ValueError("a scalar outside 0 .. r - 1")
            k32 += v.to_bytes(32, "little")
        if n == 0:
            self.last_evolve_stats = {"stage_ms": 0.0, "certified_slots": 0, "bad_at": []}
            return b"", []
        pm = np.ascontiguousarray(np.asarray(perms, dtype="<u4").reshape(-1))
        kbuf = (ctypes.c_char * len(k32)).from_buffer(k32)
        post = ctypes.create_string_buffer(96 * ell * n)
        st, at = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)()
        writers = np.empty((min(self.n_slots, n * ell), 2), dtype="<u4")
        nw, stats = ctypes.c_size_t(0), (ctypes.c_float * 2)()
        before = self.packed()
        try:
            self.ctx.check(N.cg1_chain_evolve_device(self.ctx.handle, self.d_pts.ptr, self.d_pstat.ptr, self.n_slots, idx.ctypes.data, pm.ctypes.data, kbuf, n, ell, post,
                                                     st, at, writers.ctypes.data, ctypes.byref(nw), stats))
            self._apply_writers(writers[: nw.value], post.raw)
        except BaseException:
            self._restore(before)
            raise
        finally:
            ctypes.memset(kbuf, 0, len(k32))
        self.last_evolve_stats = {"stage_ms": float(stats[0]), "certified_slots": int(stats[1]), "bad_at": list(at)}
        return post.raw[: 96 * ell * n], list(st)

    def _free(self) -> None:
        for b in (self.d_wire, self.d_pts, self.d_pstat):
            if b is not None:
                b.free()
        self.d_wire = self.d_pts = self.d_pstat = None
        self.n_slots = 0

    def close(self) -> None:
        """Release the device buffers.  The set must not be used afterwards.  Idempotent."""
        self._free()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShuffleChainVerifier:
    """Blocks of a shuffle chain, (indices, post trackers, proof) each, verified in order against a TrackerSet (module docstring).

    verify_blocks(blocks)                              object form: indices as a sequence of ell ints, post trackers as
                                                       ShuffleBatchVerifier.pack takes them (WhiskTracker-likes or byte pairs), proof bytes
    verify_blocks_packed(indices, posts, proofs, n)    wire form: n x ell slot indices (ints, or uint32 little-endian bytes), n x ell x
                                                       (r_G | k_r_G), n x crs.proof_bytes
    Both return the per-block status list (0 = valid) and leave it in `last_status`; `last_stats` carries the inner verifier's statistics
    summed over the internal batches plus "decoded_points", "gathered_points" and "valid_prefix".  An index outside the set, or a block with
    another number of indices or post trackers than ell, is the caller's error: ValueError, and the set stays as it was.

    Calls of more than 2 SPLIT blocks are cut into internal batches of SPLIT, as ShuffleBatchVerifier.verify_packed cuts them; a later batch
    finds what an earlier one wrote in the resident set.

    Throughput (profiles/r20_chain_verify_timing.txt; ell = 124, 4 hardware queues): 7.9-8.2e4 blocks/s with SPLIT = 1 024 on the instance
    (6.6e4 with the class's 2 048 over 8 192 blocks) against 8.0-8.1e4 for the expanded blocks on a one-pipeline ShuffleBatchVerifier -- no
    difference -- and 1.36-1.38e5 on the default one, which coalesces to 4 096 proofs per front-end launch: this path beats neither.  Where
    the blocks can be expanded on the host and throughput is what counts, use ShuffleBatchVerifier."""

    SPLIT = ShuffleBatchVerifier.SPLIT

    def __init__(self, crs, tracker_set: TrackerSet, device_front_end: Optional[bool] = None, threads: int = 0, chunk: int = 256, **verifier_args):
        self.set = tracker_set
        self.verifier = ShuffleBatchVerifier(crs, tracker_set.ctx, threads=threads, chunk=chunk, device_front_end=device_front_end, pipelines=1, coalesce=0,
                                             **verifier_args)
        self.crs = self.verifier.crs
        self.last_status: List[int] = []
        self.last_stats: dict = {}

    def close(self) -> None:
        self.verifier.close()

    def verify_blocks(self, blocks, mode: str = "merged", rng=None) -> List[int]:
        ell, pb = self.crs.ell, self.crs.proof_bytes
        idx, posts, proofs, pre_status = [], [], [], []
        for indices, post, proof in blocks:
            indices, post, proof = list(indices), list(post), bytes(proof)
            if len(indices) != ell or len(post) != ell:
                raise ValueError(f"a block names {len(indices)} slots and {len(post)} post trackers, not {ell}")
            idx += [int(i) for i in indices]
            posts.append(_packed_trackers(post))
            ok = len(proof) >= pb                                  # (trailing bytes are never read: ShuffleBatchVerifier.pack)
            proofs.append(proof[:pb] if ok else bytes(pb))
            pre_status.append(0 if ok else REJECT_LENGTH)
        return self.verify_blocks_packed(idx, b"".join(posts), b"".join(proofs), len(proofs), mode=mode, rng=rng, pre_status=pre_status if any(pre_status) else None)

    def _pieces(self, idx, posts: bytes, proofs: bytes, n: int, pre_status, weights):
        """The call's internal batches as the inner verifier's stream takes them: each expanded against the set's host bytes as the batches
        before it left them, with its chain plan as the Batch's `chain`."""
        import numpy as np

        ts, ell, L, pb = self.set, self.crs.ell, self.crs.points_per_proof, self.crs.proof_bytes
        step = self.SPLIT if n > 2 * self.SPLIT else n
        prf, w = memoryview(proofs), (memoryview(weights) if weights is not None else None)
        for a in range(0, n, step):
            m = min(step, n - a)
            inst = ctypes.create_string_buffer(m * 4 * ell * 48)
            plan = (ctypes.c_int32 * (m * 2 * ell))()
            writers = np.empty((min(ts.n_slots, m * ell), 2), dtype="<u4")
            nw = ctypes.c_size_t(0)
            rc = N.cg1_chain_expand(ts._host, ts.n_slots, idx[a * ell:].ctypes.data, _addr_of(posts) + a * ell * 96, m, ell, L, inst, plan, writers.ctypes.data,
                                    ctypes.byref(nw))
            if rc:
                raise N.NativeError(f"cg1_chain_expand failed ({rc})")
            writers = writers[: nw.value].astype(np.int64)
            src = (writers[:, 1] // ell) * L + 2 * ell + writers[:, 1] % ell      # the T position of the slot's last writer; U lies ell further
            pairs = np.empty((2 * nw.value, 2), dtype="<u4")
            pairs[0::2, 0], pairs[1::2, 0] = 2 * writers[:, 0], 2 * writers[:, 0] + 1
            pairs[0::2, 1], pairs[1::2, 1] = src, src + ell
            chain = {"set": ts, "plan": plan, "pairs": pairs.tobytes(), "n_pairs": 2 * nw.value, "decoded_points": 0, "gathered_points": 0}
            yield Batch(inst, proofs if m == n else bytes(prf[a * pb: (a + m) * pb]), m, None if pre_status is None else list(pre_status[a: a + m]),
                        None if w is None else bytes(w[a * 12 * 32: (a + m) * 12 * 32]), chain)

    def verify_blocks_packed(self, indices, posts: bytes, proofs: bytes, n: int, mode: str = "merged", rng=None, weights=None, pre_status=None) -> List[int]:
        import numpy as np

        ts, ell, L, pb = self.set, self.crs.ell, self.crs.points_per_proof, self.crs.proof_bytes
        if isinstance(indices, (bytes, bytearray, memoryview)):
            idx = np.frombuffer(bytes(indices), dtype="<u4")
        else:
            wide = np.asarray(indices, dtype=np.int64).reshape(-1)
            if len(wide) and (wide.min() < 0 or wide.max() >= ts.n_slots):
                raise ValueError(f"a slot index outside the set of {ts.n_slots}")
            idx = wide.astype("<u4")
        idx = np.ascontiguousarray(idx)
        posts, proofs = bytes(posts), bytes(proofs)
        if len(idx) != n * ell or len(posts) != n * ell * 96 or len(proofs) != n * pb:
            raise ValueError("verify_blocks_packed: expected n x ell indices, n x ell x 96 post bytes and n x proof_bytes")
        if len(idx) and int(idx.max()) >= ts.n_slots:
            raise ValueError(f"a slot index outside the set of {ts.n_slots}")
        if n == 0:
            self.last_status, self.last_stats = [], {"decoded_points": 0, "gathered_points": 0, "valid_prefix": 0}
            return []
        before = ts.packed()
        out: List[int] = []
        total: dict = {}
        try:
            for st in self.verifier.verify_stream(self._pieces(idx, posts, proofs, n, pre_status, weights), mode=mode, rng=rng):
                out += st
                sum_stats(total, self.verifier.last_stats)             # the call's statistics: summed over its internal batches
            prefix = next((i for i, s in enumerate(out) if s), n)
            if prefix < n:
                # rare, and allowed to be slow: the host bytes are authoritative -- the prefix replayed over the state before the call --
                # and only the slots a block behind the prefix wrote are decoded again
                ctypes.memmove(ts._host, before, len(before))
                rc = N.cg1_chain_expand(ts._host, ts.n_slots, idx.ctypes.data, posts, prefix, ell, L, None, None, None, None)
                if rc:
                    raise N.NativeError(f"cg1_chain_expand failed ({rc})")
                ts._reload_slots(np.unique(idx[prefix * ell:]))
        except BaseException:
            ctypes.memmove(ts._host, before, len(before))          # whatever was in flight: back to the state before the call, decoded afresh
            try:
                ts.ctx.check(N.cg1_stream_sync(ts.ctx.handle))
                ts._load()
            except Exception:
                pass
            raise
        total["valid_prefix"] = prefix
        self.last_status, self.last_stats = out, total
        return out


def _addr_of(b: bytes) -> int:
    return ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value


class ShuffleChainProver:
    """A chain of Whisk shuffles PROVED over a TrackerSet: `ell` slot indices per block and a seed in, blocks ready for
    ShuffleChainVerifier.verify_blocks out, the set advanced on host and device.

    prove_blocks(index_lists, seed=None, first_index=0)          -> [(indices, post_trackers, proof_bytes) or None where refused, ...]
    prove_blocks_packed(indices, n, seed=None, first_index=0)    -> (post96, proofs, status): n x ell x (T48 | U48), n x (M || proof), a list
    Both leave `last_status`, `last_refusals` ((tracker index, "r_G" | "k_r_G") or None per block, as ShuffleBatchProver's) and `last_stats`.

    Block j, for j = 0 .. n - 1 in order, reads pre_j = [set[i] for i in indices_j] before any of its own writes.  Its outputs ARE item 0 of
    ShuffleBatchProver.generate_packed(pre_j as 96 ell bytes, seed, first_index=first_index + j): the same post bytes, the same M || proof
    bytes, the same status.  If the status is 0 it writes set[indices_j[t]] = post_j[t] for t = 0 .. ell - 1 in order (indices may repeat:
    the last write wins) -- ShuffleChainVerifier's semantics.  A block whose pre trackers hold a point that does not decode gets status 2,
    one with a pre point outside G1 status 3; a refused block gets zero bytes in both outputs (None on the list face), and it WRITES
    NOTHING: later blocks are proved as if it were not there, but under their own index first_index + j.  So the output does not depend on
    how a call is cut: prove_blocks(all) == prove_blocks(head) followed by prove_blocks(tail, first_index=first_index + len(head)).

    seed=None draws secrets.token_bytes(32); the warning of ShuffleBatchProver.generate_packed about seeds holds here word for word.
    ValueError (an index outside the set, a wrong count of indices, a closed prover or set) before anything runs, the set as it was.
    NativeError: host bytes and device records are as they were before the call.

    How (cg1_chain_prove_seeded, csrc/capi_chain_prove.h): the draws of all blocks first; the distinct slots the call reads are certified in
    G1; a host pass (csrc/chain_lineage.h) names for every pre and post position its origin slot and the product of the k's on the way;
    ONE launch (k_chain_lineage_mul) makes every tracker of every block; the proofs, independent now, run through the whole-shuffle chain
    in groups of 64.  Calls of more than MAX_BLOCKS blocks go as further native calls; the cut invariance makes that free.  The device work
    runs on the TABLE's context, which must sit on the set's device; one caller at a time."""

    MAX_BLOCKS = N.WHISK_SHUFFLE_DRAWS_MAX_PROVERS

    def __init__(self, crs, tracker_set: TrackerSet, table=None):
        from .shuffle_prover import ShuffleBatchProver

        self.set = tracker_set
        self._prover = ShuffleBatchProver(crs, table=table)
        self.crs, self.ell = crs, self._prover.ell
        self.last_status: List[int] = []
        self.last_refusals: list = []
        self.last_stats: dict = {}

    def close(self) -> None:
        """Release the table when this prover made it.  The tracker set stays the caller's.  Idempotent."""
        self._prover.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def prove_blocks(self, index_lists, seed: Optional[bytes] = None, first_index: int = 0):
        ell = self.ell
        index_lists = [[int(i) for i in block] for block in index_lists]
        for block in index_lists:
            if len(block) != ell:
                raise ValueError(f"a block names {len(block)} slots, not {ell}")
        post, proofs, status = self.prove_blocks_packed([i for block in index_lists for i in block], len(index_lists), seed, first_index)
        wb = len(proofs) // max(1, len(status))
        out = []
        for j, st in enumerate(status):
            rec = post[96 * ell * j: 96 * ell * (j + 1)]
            out.append(None if st else (index_lists[j], [(rec[96 * i: 96 * i + 48], rec[96 * i + 48: 96 * i + 96]) for i in range(ell)], proofs[wb * j: wb * (j + 1)]))
        return out

    def prove_blocks_packed(self, indices, n: int, seed: Optional[bytes] = None, first_index: int = 0):
        import secrets

        import numpy as np

        from .shuffle_prover import HALF_NAMES

        ts, ell, table = self.set, self.ell, self._prover.table
        if table is None:
            raise ValueError("the prover is closed")
        ts._check_open()
        idx, n_idx = ts._indices(indices, ell)
        if n_idx != n:
            raise ValueError(f"prove_blocks_packed: expected n x ell = {n * ell} indices")
        if seed is None:
            seed = secrets.token_bytes(32)
        seed = bytes(seed)
        if len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        if isinstance(first_index, bool) or not isinstance(first_index, int) or first_index < 0 or first_index + n > 1 << 32:
            raise ValueError("first_index: an int with first_index + the number of blocks <= 2^32")
        self.last_status, self.last_refusals = [], []
        self.last_stats = {"stage_ms": 0.0, "certified_slots": 0, "chain_ms": 0.0, "call_ms": 0.0, "native_calls": 0}
        if n == 0:
            return b"", b"", []
        wb = int(N.cg1_whisk_shuffle_proof_bytes(ell))
        posts, proofs, status, refusals = [], [], [], []
        stats = dict(self.last_stats)
        before = ts.packed()
        try:
            with table._ctx_lock():
                if table._KIND != "fixed-base":
                    raise TypeError("the device pipeline of a shuffle proof runs over a FixedBaseTable")
                cx = table._ctx
                if int(N.cg1_ctx_device(cx.handle)) != int(N.cg1_ctx_device(ts.ctx.handle)):
                    raise ValueError("the table and the tracker set sit on different devices")
                gi, hi, ui, gti, gui, gth = self._prover._crs_args()
                g_arr, h_arr = (ctypes.c_uint32 * ell)(*gi), (ctypes.c_uint32 * 4)(*hi)
                ts.ctx.check(N.cg1_stream_sync(ts.ctx.handle))                # whatever the set's own stream still holds, before another stream touches it
                for lo in range(0, n, self.MAX_BLOCKS):
                    m = min(self.MAX_BLOCKS, n - lo)
                    post, out = ctypes.create_string_buffer(96 * ell * m), ctypes.create_string_buffer(wb * m)
                    st, at = (ctypes.c_int32 * m)(), (ctypes.c_uint32 * m)()
                    writers = np.empty((min(ts.n_slots, m * ell), 2), dtype="<u4")
                    nw, fl = ctypes.c_size_t(0), (ctypes.c_float * 4)()
                    cx.check(N.cg1_chain_prove_seeded(cx.handle, table._tab.handle, ell, m, g_arr, h_arr, ui, gti, gui, gth, ts.d_pts.ptr, ts.d_pstat.ptr, ts.n_slots,
                                                      idx[lo * ell:].ctypes.data, seed, first_index + lo, post, out, st, at, writers.ctypes.data, ctypes.byref(nw), fl))
                    ts._apply_writers(writers[: nw.value], post.raw)
                    posts.append(post.raw[: 96 * ell * m]); proofs.append(out.raw[: wb * m]); status += list(st)
                    refusals += [(a >> 1, HALF_NAMES[a & 1]) if s else None for s, a in zip(st, at)]
                    stats["stage_ms"] += float(fl[0]); stats["certified_slots"] += int(fl[1]); stats["chain_ms"] += float(fl[2]); stats["call_ms"] += float(fl[3])
                    stats["native_calls"] += 1
        except BaseException:
            ts._restore(before)
            raise
        self.last_status, self.last_refusals, self.last_stats = status, refusals, stats
        return b"".join(posts), b"".join(proofs), list(status)
