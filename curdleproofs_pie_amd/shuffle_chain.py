"""A chain of Whisk shuffles verified over a tracker set that stays on the device in decoded form.

Whisk produces its shuffles as a chain over ONE candidate set: N trackers (16 384 in the consensus spec); every block names `ell` slots of
it, proves a shuffle of what lies there and writes its post trackers back into the same slots.  After the first touch of a slot every pre
tracker of a block is the post tracker of an earlier block.  `ShuffleBatchVerifier` takes self-contained items (pre, post, proof) and decodes
all 4 ell + 89 points of each -- a square root per point, the verifier's dominant kernel -- although the 2 ell pre trackers were decoded
moments earlier as somebody's posts.  Here they are decoded once:

    TrackerSet            the N trackers as host bytes (authoritative) and as 2 N decoded records + status bytes on the device
    ShuffleChainVerifier  blocks as (indices, post trackers, proof) against a TrackerSet

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
        before it left them, with its chain plan as the ticket's sixth field."""
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
            yield (inst, proofs if m == n else bytes(prf[a * pb: (a + m) * pb]), m, None if pre_status is None else list(pre_status[a: a + m]),
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
                for k, v in (self.verifier.last_stats or {}).items():      # the call's statistics: summed over its internal batches
                    if isinstance(v, bool) or not isinstance(v, (int, float)):
                        total[k] = v
                    else:
                        total[k] = total.get(k, 0) + v
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
