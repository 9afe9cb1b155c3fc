"""The shuffle verifier's plumbing without a GPU (curdleproofs_pie_amd/verifier_pipeline.py): the batch type, the rule by which a stream's
batches travel together, the table of a slot's buffer sizes, and the ticket's one error channel behind the stage runner."""
import json
import os
import random
import sys
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from curdleproofs_pie_amd import _native as N  # noqa: E402
from curdleproofs_pie_amd.shuffle_verifier import ShuffleBatchVerifier, ShuffleCrs  # noqa: E402
from curdleproofs_pie_amd.verifier_pipeline import Batch, Lanes, Slot, Ticket, coalesce_plan, sum_stats  # noqa: E402

LIMIT = 4096


# ---------------------------------------------------------------- Batch
def test_batch_of_round_trips_tuples_and_batches():
    full = (b"i", b"p", 1, [0], b"w", {"plan": 1})
    for k in (3, 4, 5, 6):
        b = Batch.of(full[:k])
        assert (b.instances, b.proofs, b.n, b.pre_status, b.weights, b.chain) == full[:k] + (None,) * (6 - k)
        assert b.plain is (k == 3)
        assert Batch.of(b) is b
        assert Batch.of(list(full[:k])) == b
    for k in (2, 7):
        with pytest.raises(ValueError):
            Batch.of((full + (None,))[:k])
    with pytest.raises(AttributeError):
        Batch.of(full).wieghts = b""                             # a mistyped field is an error, not a new key


def test_weights_filled_in_keep_the_chain_plan():
    plan = {"plan": 1}
    b = Batch.of((b"i", b"p", 1, None, None, plan))
    w = b.with_weights(b"w")
    assert w.weights == b"w" and w.chain is plan and (w.instances, w.proofs, w.n, w.pre_status) == (b"i", b"p", 1, None)
    assert b.weights is None                                     # the caller's batch is left as it was


# ---------------------------------------------------------------- the coalescing plan
def plain(n):
    return Batch.of((bytes(n), bytes(2 * n), n))                 # one byte per instance, two per proof


def own(n):
    return Batch.of((bytes(n), bytes(2 * n), n, [0] * n))


def plan_of(batches):
    return list(coalesce_plan(iter(batches), LIMIT, 1, 2))


def test_coalescing_groups():
    sizes = lambda batches: [s for _, s in plan_of(batches)]
    assert sizes([plain(1024) for _ in range(5)]) == [[1024] * 4, [1024]]
    assert sizes([plain(1024), plain(4096), plain(1024)]) == [[1024], [4096], [1024]]
    assert sizes([plain(3000), plain(2000)]) == [[3000], [2000]]
    assert plan_of([]) == []
    mine = own(512)
    groups = plan_of([plain(1024), mine, plain(1024)])
    assert [s for _, s in groups] == [[1024], [512], [1024]] and groups[1][0] is mine
    big = plain(4096)
    assert plan_of([big])[0][0] is big                           # alone: the caller's own object, nothing wrapped


def test_a_group_travels_as_segments_of_its_members():
    members = [Batch.of((bytes([k]) * n, bytes([k]) * (2 * n), n)) for k, n in enumerate((1000, 24, 3000))]
    (batch, sizes), = plan_of(members)
    assert sizes == [1000, 24, 3000] and batch.n == 4024 and batch.plain
    assert len(batch.instances) == 4024 and len(batch.proofs) == 2 * 4024
    assert batch.instances.joined() == b"".join(m.instances for m in members) and batch.proofs.joined() == b"".join(m.proofs for m in members)
    assert [(a, cnt) for _, a, cnt in batch.proofs.runs(990, 1030)] == [(990, 10), (1000, 24), (1024, 6)]


def test_coalescing_properties_on_a_random_stream():
    rng = random.Random(20260101)
    stream = [own(n) if k % 7 == 6 else plain(n) for k, n in enumerate(rng.randint(1, 5000) for _ in range(200))]
    pulled = []

    def feed():
        for b in stream:
            pulled.append(b)
            yield b

    seen, multi = [], 0
    for batch, sizes in coalesce_plan(feed(), LIMIT, 1, 2):
        members = stream[len(seen): len(seen) + len(sizes)]
        assert sizes == [m.n for m in members] and batch.n == sum(sizes)           # the input order, nothing dropped or repeated
        seen += members
        assert len(pulled) <= len(seen) + 1                      # lazy: at most the one batch that closed the group was pulled beyond it
        if len(sizes) > 1:
            multi += 1
            assert sum(sizes) <= LIMIT and all(m.plain and m.n < LIMIT for m in members)
            assert batch.instances.joined() == b"".join(m.instances for m in members)
        else:
            assert batch is members[0]
    assert seen == stream and multi > 10


# ---------------------------------------------------------------- Slot.sizes
@pytest.fixture(scope="module")
def dims():
    with open(os.path.join(ROOT, "tests", "golden", "shuffle_vectors.json")) as f:
        crs = ShuffleCrs(bytes.fromhex(json.load(f)["cases"][0]["crs"]))
    return crs.points_per_proof, crs.ncrs, int(N.cg1_shuffle_rowin_scalars(crs.handle))


@pytest.mark.parametrize("n", [1, 8, 9, 1024])
def test_slot_sizes(dims, n):
    L, C, K = dims
    table = Slot.sizes(n, L, C, K, ShuffleBatchVerifier.FE_FIRST_MAX)
    assert ShuffleBatchVerifier.FE_FIRST_MAX == 8
    assert sum(table["pinned"].values()) == n * L * 48 + (n * L + C) * 32 + n * K * 32 + 4 * n + n * L + 768 * n + min(n, 8) * L * 48
    assert sorted(table["device"]) == sorted(["wire", "pts", "pstat", "sgflags", "sc", "rowin", "hstat", "csrows", "dstat"])
    assert table["device"]["pts"] == (n * L + C) * 96 and table["device"]["sc"] == (n * L + C) * 32 and table["device"]["sgflags"] == 10 * n
    assert all(v > 0 for group in table.values() for v in group.values())


# ---------------------------------------------------------------- Ticket and the stage runner
class Boom(Exception):
    pass


def ticket():
    return Ticket(Batch.of((b"", b"", 2)), None, "merged", [(0, 1), (1, 2)])


def test_a_failing_stage_reaches_every_waiter_and_the_lane_goes_on():
    lanes, tk, first = Lanes(1), ticket(), Boom("first")
    try:
        def stage():
            tk.chunks.put((0, 1))
            raise first

        lanes.stage(0, tk, tk.flags_done, stage)
        assert tk.next_chunk() == (0, 1)                         # what was decoded before the failure is still handed out, in order
        for waiter in (tk.next_chunk, tk.next_chunk, tk.flags, tk.result, lambda: tk.wait(tk.fe_done)):
            with pytest.raises(Boom) as e:
                waiter()
            assert e.value is first
        assert tk.done.is_set() and tk.flags_done.is_set() and tk.fe_done.is_set() and tk.error is first
        tk.fail(Boom("second"))
        assert tk.error is first
        with pytest.raises(Boom) as e:
            tk.result()
        assert e.value is first
        # the lane's thread survived: the next ticket's stage runs on it
        nxt, ran = ticket(), []
        lanes.stage(0, nxt, nxt.done, lambda: ran.append(threading.current_thread()))
        assert nxt.done.wait(5) and ran == [lanes.threads[0]]
    finally:
        lanes.stop()
    assert lanes.threads == [None]


def test_a_stage_that_succeeds_leaves_no_error():
    lanes, tk = Lanes(2), ticket()
    try:
        def decode():
            for r in tk.bounds:
                tk.chunks.put(r)
            tk.sgflags = bytes(20)

        def msm():
            assert [tk.next_chunk(), tk.next_chunk()] == tk.bounds and tk.flags() == bytes(20)
            tk.status = [0, 6]

        lanes.stage(1, tk, tk.done, msm)                         # waits on lane 1 for what lane 0 produces
        lanes.stage(0, tk, tk.flags_done, decode)
        assert tk.result() == [0, 6] and tk.error is None and not tk.fe_done.is_set()
    finally:
        lanes.stop()
    with pytest.raises(AttributeError):
        tk.statuss = []                                          # a mistyped field is an error


def test_sum_stats():
    total = {}
    for piece in ({"n": 2, "t": 0.5, "merged_ok": True, "exact_path": None}, None, {"n": 3, "t": 0.25, "merged_ok": False, "exact_path": "host"}):
        sum_stats(total, piece)
    assert total == {"n": 5, "t": 0.75, "merged_ok": False, "exact_path": "host"}
