"""What travels through the shuffle verifier's stages (shuffle_verifier.py), apart from the verifier itself: a caller's `Batch`, the `Ticket`
of a batch in flight with its one error channel, the `Slot` of buffers it occupies and the table of their sizes, the `Lanes` its stages
run on, and the rule by which a stream's batches travel together (`coalesce_plan`).  Nothing here makes a verifier's native call: buffers
are allocated and freed, nothing else, so all of it but a Slot's allocation runs without a GPU."""
from __future__ import annotations

import ctypes
import queue
import threading
import time
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Optional, Sequence

from . import _native as N

N_EXACT_POINTS = 10            # T_1 T_2 U_1 U_2 R S cm_A cm_B: the proof's points in the same-scalar equalities (same_scalar.py:82-108)


def _addr(b) -> int:
    """Address of the first byte of a bytes object / ctypes buffer (to pass sub-ranges of a batch to native code)."""
    if isinstance(b, bytes):
        return ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value
    return ctypes.addressof(b)


class _Segments:
    """Several callers' batches travelling as ONE internal batch without being copied together: item i of the internal batch is item
    i - first of the segment that holds it.  `runs(lo, hi)` cuts [lo, hi) at the segment boundaries."""

    def __init__(self, parts, item_bytes: int):
        self.parts = list(parts)                              # [(bytes-like, n_items)]
        self.item_bytes = item_bytes
        self.first = [0]
        for _, n in self.parts:
            self.first.append(self.first[-1] + n)

    def __len__(self) -> int:
        return self.first[-1] * self.item_bytes

    def runs(self, lo: int, hi: int):
        """(address of item `a`, a, count) for every maximal run [a, a + count) of [lo, hi) inside one segment"""
        for k, (buf, n) in enumerate(self.parts):
            f = self.first[k]
            a, b = max(lo, f), min(hi, f + n)
            if a < b:
                yield _addr(buf) + (a - f) * self.item_bytes, a, b - a

    def item_addr(self, i: int) -> int:
        for addr, a, cnt in self.runs(i, i + 1):
            return addr
        raise IndexError(i)

    def joined(self) -> bytes:
        return b"".join(bytes(buf) for buf, _ in self.parts)


def _runs(buf, item_bytes: int, lo: int, hi: int):
    """The same for a plain contiguous buffer: one run."""
    if isinstance(buf, _Segments):
        yield from buf.runs(lo, hi)
    else:
        yield _addr(buf) + lo * item_bytes, lo, hi - lo


@dataclass(slots=True)
class Batch:
    """One batch of a stream: n proofs in wire form, and what the caller may add to them -- reject codes from packing, weights, a chain plan
    (shuffle_chain.py).  `plain`: the caller gave nothing but the first three, so the batch may travel with its neighbours (coalesce_plan)."""
    instances: object
    proofs: object
    n: int
    pre_status: Optional[Sequence[int]] = None
    weights: Optional[bytes] = None
    chain: Optional[dict] = None
    plain: bool = False

    @classmethod
    def of(cls, x) -> "Batch":
        """A Batch as it is; the tuple form of verify_stream, (instances, proofs, n[, pre_status[, weights[, chain plan]]]), as a Batch."""
        if isinstance(x, Batch):
            return x
        x = tuple(x)
        if not 3 <= len(x) <= 6:
            raise ValueError(f"a batch is (instances, proofs, n[, pre_status[, weights[, chain plan]]]), not {len(x)} items")
        return cls(*x, plain=len(x) == 3)

    def with_weights(self, weights: bytes) -> "Batch":
        return replace(self, weights=weights, plain=False)


def coalesce_plan(batches, limit: int, instance_bytes: int, proof_bytes: int):
    """(internal batch, [sizes of the callers' batches inside it]) for a stream of Batches: consecutive plain batches travel together, up to
    `limit` proofs per internal batch; a batch that is not plain, or has `limit` proofs or more, goes through alone and as the caller's own
    object.  Lazy: a group is yielded as soon as it is full or the batch behind it cannot join, so at most that one batch is pulled from
    `batches` beyond the groups already yielded.  The members are NOT copied together: the stages gather from the segments where they lie."""
    def flush():
        if len(pend) == 1:
            return pend[0], [pend[0].n]
        for x in pend:
            assert len(x.instances) == x.n * instance_bytes and len(x.proofs) == x.n * proof_bytes
        sizes = [x.n for x in pend]
        return Batch(_Segments([(x.instances, x.n) for x in pend], instance_bytes), _Segments([(x.proofs, x.n) for x in pend], proof_bytes),
                     sum(sizes), plain=True), sizes

    pend, size = [], 0
    for b in batches:
        alone = not b.plain or b.n >= limit
        if pend and (alone or size + b.n > limit):
            yield flush()
            pend, size = [], 0
        if alone:
            yield b, [b.n]
            continue
        pend.append(b)
        size += b.n
        if size >= limit:
            yield flush()
            pend, size = [], 0
    if pend:
        yield flush()


def sum_stats(total: dict, stats: Optional[dict]) -> None:
    """A call's statistics, summed over its pieces: numbers add up, everything else (flags, names, None) keeps the last piece's value."""
    for k, v in (stats or {}).items():
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            total[k] = v
        else:
            total[k] = total.get(k, 0) + v


class Ticket:
    """One batch in flight: its slot, what the stages hand each other, and ONE error channel.  Three threads write to it -- the decoding
    lane (chunks, decompress_s, sgflags, flags_done), the front-end (device_rows, prep, front_end_s, fe_done) and the MSM lane (status,
    stats, done); whichever fails first calls fail(), which releases every wait of the others with that exception."""
    __slots__ = ("slot", "n", "instances", "proofs", "pre_status", "weights", "chain", "mode", "bounds", "fe_first", "device_rows", "prep",
                 "sgflags", "status", "stats", "t0", "decompress_s", "front_end_s", "chunks", "flags_done", "fe_done", "done", "error", "_lock")

    def __init__(self, batch: Batch, slot, mode: str, bounds, fe_first: bool = False):
        self.slot, self.mode, self.bounds, self.fe_first = slot, mode, bounds, fe_first
        self.n, self.instances, self.proofs = batch.n, batch.instances, batch.proofs
        self.pre_status, self.weights, self.chain = batch.pre_status, batch.weights, batch.chain
        self.device_rows, self.prep, self.sgflags, self.status, self.stats = True, None, None, None, None
        self.t0, self.decompress_s, self.front_end_s = time.perf_counter(), 0.0, 0.0
        self.chunks = queue.Queue()                           # (lo, hi) of every decoded sub-batch, in order
        self.flags_done, self.fe_done, self.done = threading.Event(), threading.Event(), threading.Event()
        self.error, self._lock = None, threading.Lock()

    def fail(self, exc: BaseException) -> None:
        """Record the first exception and release everyone who waits for this ticket (chunks, flags, front-end, done)."""
        with self._lock:
            if self.error is None:
                self.error = exc
        self.chunks.put(None)
        for ev in (self.flags_done, self.fe_done, self.done):
            ev.set()

    def next_chunk(self):
        """Bounds of the next decoded sub-batch; raises what a stage recorded."""
        r = self.chunks.get()
        if r is None:
            self.chunks.put(None)                             # (for whoever asks again)
            raise self.error
        return r

    def wait(self, event: threading.Event) -> None:
        """For one of the ticket's three events; raises what a stage recorded."""
        event.wait()
        if self.error is not None:
            raise self.error

    def flags(self):
        """The subgroup flags, once the decoding lane has brought them back."""
        self.wait(self.flags_done)
        return self.sgflags

    def result(self):
        """The batch's status list, once its last stage has ended."""
        self.wait(self.done)
        return self.status


class Lanes:
    """GPU work runs on persistent threads (a thread's first HIP call is expensive; a context takes one call at a time), one job queue
    each, started on first use: lane 0 drives `ctx` (staging + decompression, in submission order), lane 1 drives `ctx_msm` (MSMs), lane
    2 + k the k-th front-end launch context."""

    def __init__(self, count: int):
        self.threads, self.jobs = [None] * count, [None] * count

    def submit(self, fn, lane: int = 0) -> None:
        if self.threads[lane] is None:
            jobs = self.jobs[lane] = queue.Queue()

            def loop(jobs=jobs):
                while True:
                    job = jobs.get()
                    if job is None:
                        return
                    job()

            self.threads[lane] = threading.Thread(target=loop, daemon=True)
            self.threads[lane].start()
        self.jobs[lane].put(fn)

    def stage(self, lane: int, ticket: Ticket, event: threading.Event, fn) -> None:
        """A stage of `ticket` on `lane`: whatever it raises goes to ticket.fail (surfaced in the consumer); `event` is set when it ends."""
        def job():
            try:
                fn()
            except BaseException as e:
                ticket.fail(e)
            finally:
                event.set()

        self.submit(job, lane)

    def stop(self) -> None:
        """After what is queued has drained."""
        for lane, t in enumerate(self.threads):
            if t is not None:
                self.jobs[lane].put(None)
                t.join()
            self.threads[lane] = self.jobs[lane] = None


class Slot:
    """Buffers of one batch in flight, three groups apart: `dev` (device), `pin` (page-locked staging) and `scratch` (plain host buffers that
    `Prepared` makes once and reuses); `exact` is the device group of the exact-relations pass, made when a batch first needs it.  Every size
    is an entry of `Slot.sizes`: allocation, the byte counts and free() all go by that table."""
    __slots__ = ("cap", "busy", "crs_at", "table", "dev", "pin", "scratch", "exact")

    @staticmethod
    def sizes(n: int, L: int, C: int, K: int, fe_first_max: int) -> dict:
        """group -> name -> bytes for n proofs of L own points and K row-input scalars each over C CRS points."""
        return {
            "device": {
                "wire": n * L * 48,
                "pts": (n * L + C) * 96,                     # own points of all proofs, then the CRS points
                "pstat": n * L,
                "sgflags": n * N_EXACT_POINTS,               # 1 = outside G1, for the points of the exactly-asserted equalities
                "sc": (n * L + C) * 32,
                "rowin": n * K * 32,                         # device row builder: input blocks, host codes, CRS rows, final codes
                "hstat": 4 * n, "csrows": n * C * 32, "dstat": 4 * n},
            "pinned": {
                "wire": n * L * 48, "sc": (n * L + C) * 32, "rowin": n * K * 32, "hstat": 4 * n, "pstat": n * L, "decoded": n * 768,
                "fe_wire": min(n, fe_first_max) * L * 48},   # the front-end's own copy of a tiny batch's points
            "exact": {
                "ok": 4 * n, "rowin": n * K * 32, "pts": n * L * 96, "rep": n * C * 96, "sc": (n * L + C) * 32, "csrows": n * C * 32,
                "dstat": 4 * n, "hstat": 4 * n, "pstat": n * L}}

    def __init__(self, ctx, n: int, L: int, C: int, K: int, fe_first_max: int):
        self.cap, self.busy, self.crs_at, self.exact = n, None, None, None
        self.table = Slot.sizes(n, L, C, K, fe_first_max)
        self.dev = SimpleNamespace(**{k: ctx.alloc(v) for k, v in self.table["device"].items()})
        self.pin = SimpleNamespace(**{k: N.PinnedBuffer(ctx, v) for k, v in self.table["pinned"].items()})
        self.scratch = SimpleNamespace(crs_scalars=None, status=None)

    def exact_buffers(self, ctx):
        """Allocated once, at the slot's capacity, on the context of the lane that runs the pass."""
        if self.exact is None:
            self.exact = x = SimpleNamespace(**{k: ctx.alloc(v) for k, v in self.table["exact"].items()})
            x.hstat.upload(bytes(x.hstat.nbytes)); x.pstat.upload(bytes(x.pstat.nbytes))      # live proofs, decodable points: never written again
        return self.exact

    @property
    def pinned_bytes(self) -> int:
        return sum(self.table["pinned"].values())

    @property
    def device_bytes(self) -> int:
        return sum(self.table["device"].values())

    def free(self) -> None:
        for group in (self.dev, self.exact, self.pin):
            for buf in vars(group).values() if group is not None else ():
                buf.free()
        self.exact = None
