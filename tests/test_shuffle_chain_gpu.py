"""A chain of Whisk shuffles verified over a device-resident tracker set (curdleproofs_pie_amd/shuffle_chain.py; the strided decoding and
the record moves: csrc/kernels_batch.h, csrc/kernels_tracker_set.h, csrc/capi_tracker_set.h).  Needs an MI355X.

The kernels alone first: the strided decoding against the plain one on the taken positions with the skipped ones left as they were, the
gather and the scatter over known records.  Then whole chains at ell = 4 (and one at ell = 12 and at ell = 124) over the CRS of
tests/golden/shuffle_device_vectors.json, proved block by block against a model of the set kept here: the statuses are
ShuffleBatchVerifier.verify_packed's on the instances the model expands, the set is the model's -- host bytes and device records -- and
nothing is decoded twice."""
import ctypes
import functools
import random
import types

import pytest

from oracle import bls12_381 as O

import whisk_shuffle_cases as W

pytestmark = pytest.mark.gpu
NB = 4
SEED = bytes(range(32))
PATTERN = 0xA5


def P(enc):
    from curdleproofs_pie_amd.py_arkworks_bls12381 import G1Point
    return G1Point.from_compressed_bytes_unchecked(enc)


class SetModel:
    """The tracker set of a chain: block j reads [set[i] for i in indices_j] before any of its writes, then writes post_j[t] to
    indices_j[t] for t = 0 .. ell - 1 in order."""

    def __init__(self, trackers):
        self.slots = [(bytes(r), bytes(k)) for r, k in trackers]

    def copy(self):
        return SetModel(self.slots)

    def read(self, indices):
        return [self.slots[i] for i in indices]

    def apply(self, indices, post):
        pre = self.read(indices)
        for i, p in zip(indices, post):
            self.slots[i] = (bytes(p[0]), bytes(p[1]))
        return pre

    def packed(self):
        return b"".join(r + k for r, k in self.slots)


class Kit:
    """A fixture case's CRS as product objects over a FixedBaseTable, a prover over it, and its vec_R / vec_S encodings as trackers (as
    tests/test_whisk_shuffle_seeded_gpu.py::Kit; the case at ell = 124 stores no points: G1 * k for the scalars its seed gives first)."""

    def __init__(self, ell):
        from curdleproofs_pie_amd.fixed_base import FixedBaseTable
        from curdleproofs_pie_amd.shuffle_prover import ShuffleBatchProver

        c = next(c for c in W.golden("shuffle_device_vectors.json") if c["ell"] == ell)
        h = bytes.fromhex
        n = ell + NB
        if "vec_G" in c:
            pts = [P(h(x)) for x in c["vec_G"] + c["vec_H"] + [c["H"], c["G_t"], c["G_u"]]]
            self.pre = [(h(r), h(s)) for r, s in zip(c["vec_R"], c["vec_S"])]
        else:
            from curdleproofs_pie_amd import G1Point, Scalar
            from curdleproofs_pie_amd.msm_accumulator import batch_mul

            rng = random.Random(c["seed"])
            count = n + 3 + 2 * ell
            every = [bytes(p.to_compressed_bytes()) for p in batch_mul([G1Point()] * count, [Scalar(rng.randint(1, O.R - 1)) for _ in range(count)])]
            pts, enc = [P(e) for e in every[: n + 3]], every[n + 3:]
            self.pre = list(zip(enc[:ell], enc[ell:]))
        self.ell = ell
        self.crs = types.SimpleNamespace(vec_G=pts[:ell], vec_H=pts[ell:n], H=pts[n], G_t=pts[n + 1], G_u=pts[n + 2])
        self.table = FixedBaseTable(pts)
        self.prover = ShuffleBatchProver(self.crs, table=self.table)
        comp = lambda p: bytes(p.to_compressed_bytes())
        add = lambda v: functools.reduce(lambda a, b: a + b, v)
        self.crs_bytes = b"".join(comp(p) for p in pts + [add(self.crs.vec_G), add(self.crs.vec_H)])
        self._index = 0

    def prove(self, lists):
        """(post trackers, proof) per tracker list, every call under draws of its own"""
        got = self.prover.generate_seeded(lists, seed=SEED, first_index=self._index)
        self._index += len(lists)
        assert all(g is not None for g in got), self.prover.last_refusals
        return got

    def initial_set(self, n_slots):
        """the fixture's trackers, their swapped forms and the posts of a preliminary shuffle, repeated until the set is full"""
        base = self.pre + [(s, r) for r, s in self.pre] + self.prove([self.pre])[0][0]
        return [base[(i * 5) % len(base) if i >= len(base) else i] for i in range(n_slots)]

    def chain(self, model, index_lists):
        """The blocks (indices, post, proof) of a chain over `model`, each proved against the set as the blocks before it left it; blocks
        that read nothing an earlier block of their round wrote are proved in one call.  The model ends in the chain's final state."""
        blocks = []
        pending, dirty = [], set()
        for indices in index_lists:
            if dirty & set(indices):
                self._flush(model, pending, blocks)
                pending, dirty = [], set()
            pending.append(list(indices))
            dirty |= set(indices)
        self._flush(model, pending, blocks)
        return blocks

    def _flush(self, model, pending, blocks):
        if not pending:
            return
        for indices, (post, proof) in zip(pending, self.prove([model.read(ix) for ix in pending])):
            model.apply(indices, post)
            blocks.append((indices, post, proof))


@pytest.fixture(scope="module")
def kits(native_lib):
    made = {}

    def get(ell):
        if ell not in made:
            made[ell] = Kit(ell)
        return made[ell]

    yield get
    for k in made.values():
        k.table.close()


@pytest.fixture(scope="module")
def ctx(native_lib):
    c = native_lib.Context(0)
    yield c
    c.close()


# the 12 blocks at ell = 4 over 16 slots: block 1 reads block 0's posts (the same sub-batch at chunk = 4), block 6 reads block 2's (across
# sub-batches), block 3 names slot 8 twice, block 4 reads only untouched slots, slot 0 is written four times (blocks 0, 1, 5, 7)
INDEX_LISTS_4 = [[0, 1, 2, 3], [0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 8], [12, 13, 14, 15], [0, 11, 9, 12], [4, 5, 6, 7], [0, 1, 2, 3],
                 [15, 14, 13, 12], [3, 7, 11, 15], [8, 10, 5, 1], [2, 6, 9, 13]]


class Scenario:
    """A proved chain: the initial set, the blocks, the model's state after every block."""

    def __init__(self, kit, n_slots, index_lists):
        self.kit, self.ell = kit, kit.ell
        self.initial = kit.initial_set(n_slots)
        model = SetModel(self.initial)
        self.blocks = kit.chain(model, index_lists)
        self.final = model

    def state_after(self, blocks, start=None):
        m = SetModel(self.initial) if start is None else start.copy()
        for indices, post, _ in blocks:
            m.apply(indices, post)
        return m

    def expanded(self, blocks, start=None):
        """the items (pre, post, proof) the model expands the blocks to"""
        m = SetModel(self.initial) if start is None else start.copy()
        return [(m.apply(indices, post), post, proof) for indices, post, proof in blocks]


@pytest.fixture(scope="module")
def scenario4(kits):
    return Scenario(kits(4), 16, INDEX_LISTS_4)


@pytest.fixture(scope="module")
def reference_verifier(native_lib, kits):
    """ShuffleBatchVerifier per ell, the path the chain's statuses are defined by"""
    from curdleproofs_pie_amd.shuffle_verifier import ShuffleBatchVerifier

    made = {}

    def get(ell):
        if ell not in made:
            made[ell] = ShuffleBatchVerifier(kits(ell).crs_bytes, device_front_end=False)
        return made[ell]

    yield get
    for v in made.values():
        v.close()


def expanded_status(ref, items):
    inst, proofs, pre_status = ref.pack(items)
    return ref.verify_packed(inst, proofs, len(items), rng=random.Random(1), pre_status=pre_status)


def device_set_equals_host(N, ts):
    """the resident records and status bytes are what a plain decoding of the host bytes gives"""
    cx, n = ts.ctx, 2 * len(ts)
    d_w, d_p, d_s = cx.alloc(48 * n), cx.alloc(96 * n), cx.alloc(n)
    try:
        d_w.upload(ts.packed())
        cx.check(N.cg1_batch_decompress_device(cx.handle, d_w.ptr, d_p.ptr, d_s.ptr, n, 0))
        return ts.d_pts.download(96 * n) == d_p.download(96 * n) and ts.d_pstat.download(n) == d_s.download(n)
    finally:
        d_w.free(); d_p.free(); d_s.free()


def chain_verifier(kit, ctx, trackers, device_front_end, chunk=4):
    from curdleproofs_pie_amd.shuffle_chain import ShuffleChainVerifier, TrackerSet

    ts = TrackerSet(trackers, ctx)
    v = ShuffleChainVerifier(kit.crs_bytes, ts, device_front_end=device_front_end, chunk=chunk)
    v.verifier.prefetch_big = False          # the sub-batches stay at `chunk` proofs under both front-ends
    return ts, v


# ---------------------------------------------------------------------------------------------------- the kernels alone
def some_encodings(count):
    """valid encodings from the fixture (CRS points and trackers of the cases that store them), repeated to `count`"""
    enc = []
    for c in W.golden("shuffle_device_vectors.json"):
        if "vec_G" in c:
            enc += [bytes.fromhex(x) for x in c["vec_G"] + c["vec_H"] + c["vec_R"] + c["vec_S"] + c["vec_T"] + c["vec_U"]]
    return [enc[i % len(enc)] for i in range(count)]


@pytest.mark.parametrize("n,stride,skip,take", [(3, 7, 2, 5), (130, 3, 2, 1), (5, 61, 24, 37)])
def test_strided_decode_takes_what_it_should_and_leaves_the_rest(native_lib, ctx, n, stride, skip, take):
    """Groups straddle a 128-thread block ((130, 3, 2, 1): 130 lanes; (5, 61, 24, 37): 185) and `take` divides neither."""
    N = native_lib
    total = n * stride
    enc = some_encodings(total)
    taken = [g * stride + skip + t for g in range(n) for t in range(take)]
    enc[taken[len(taken) // 2]] = bytes(48)                      # one bad encoding among the taken positions
    d_w, d_p, d_s, d_p2, d_s2 = ctx.alloc(48 * total), ctx.alloc(96 * total), ctx.alloc(total), ctx.alloc(96 * total), ctx.alloc(total)
    try:
        d_w.upload(b"".join(enc))
        ctx.check(N.cg1_batch_decompress_device(ctx.handle, d_w.ptr, d_p2.ptr, d_s2.ptr, total, 0))
        want_p, want_s = d_p2.download(), d_s2.download()
        # the skipped positions of the wire array hold what must not be read: encodings that do not decode
        wire = bytearray(b"".join(enc))
        for i in set(range(total)) - set(taken):
            wire[48 * i: 48 * i + 48] = b"\xff" * 48
        d_w.upload(bytes(wire))
        d_p.upload(bytes([PATTERN]) * (96 * total)); d_s.upload(bytes([PATTERN]) * total)
        ctx.check(N.cg1_batch_decompress_strided_enqueue(ctx.handle, d_w.ptr, d_p.ptr, d_s.ptr, n, stride, skip, take))
        ctx.check(N.cg1_stream_sync(ctx.handle))
        got_p, got_s = d_p.download(), d_s.download()
        assert d_w.download() == bytes(wire)
    finally:
        for b in (d_w, d_p, d_s, d_p2, d_s2):
            b.free()
    bad = 0
    for i in range(total):
        if i in set(taken):
            assert got_p[96 * i: 96 * i + 96] == want_p[96 * i: 96 * i + 96] and got_s[i] == want_s[i], i
            bad += got_s[i] != 0
        else:
            assert got_p[96 * i: 96 * i + 96] == bytes([PATTERN]) * 96 and got_s[i] == PATTERN, i
    assert bad == 1
    for args in ((n, stride, stride - take + 1, take), (n, 0, 0, take), (1 << 31, stride, skip, take)):      # refused before any launch
        assert N.cg1_batch_decompress_strided_enqueue(ctx.handle, 1, 1, 1, *args) == N.ERR_ARG, args


def test_gather_and_scatter_move_records_and_status_bytes(native_lib, ctx):
    N = native_lib
    rng = random.Random(5)
    stride, take, groups, n_set = 7, 2, 3, 5
    n_pts = groups * stride
    pts, pstat = rng.randbytes(96 * n_pts), rng.randbytes(n_pts)
    spts, sstat = rng.randbytes(96 * n_set), rng.randbytes(n_set)
    d_p, d_s, d_sp, d_ss = ctx.alloc(96 * n_pts), ctx.alloc(n_pts), ctx.alloc(96 * n_set), ctx.alloc(n_set)
    rec = lambda buf, i: buf[96 * i: 96 * i + 96]
    try:
        d_p.upload(pts); d_s.upload(pstat); d_sp.upload(spts); d_ss.upload(sstat)
        # groups 1 and 2: a set entry, a decoded position of group 0, one of group 1 (earlier than group 2), the last set entry
        plan = [~0, 0 * stride + 3, 1 * stride + 5, ~4]
        arr = (ctypes.c_int32 * 4)(*plan)
        gather = lambda a, first=1, ng=2, n_points=n_pts: N.cg1_chain_gather_enqueue(ctx.handle, d_p.ptr, d_s.ptr, n_points, d_sp.ptr, d_ss.ptr, n_set, a, first, ng,
                                                                                     stride, take)
        # refusals launch nothing: a source in the group itself, a gathered position, a set entry that is not there, groups outside the array
        for bad in ([~0, 1 * stride + 3, ~1, ~2], [~0, 0 * stride + 1, ~1, ~2], [~0, ~5, ~1, ~2], [~0, n_pts, ~1, ~2]):
            assert gather((ctypes.c_int32 * 4)(*bad)) == N.ERR_ARG, bad
        assert gather(arr, first=2) == N.ERR_ARG and gather(arr, n_points=n_pts - 1) == N.ERR_ARG
        ctx.check(N.cg1_stream_sync(ctx.handle))
        assert d_p.download() == pts and d_s.download() == pstat
        ctx.check(gather(arr))
        ctx.check(N.cg1_stream_sync(ctx.handle))
        got_p, got_s = d_p.download(), d_s.download()
        want_p, want_s = bytearray(pts), bytearray(pstat)
        for dst, (src_buf, src_stat, src) in zip((7, 8, 14, 15), ((spts, sstat, 0), (pts, pstat, 3), (pts, pstat, 12), (spts, sstat, 4))):
            want_p[96 * dst: 96 * dst + 96] = rec(src_buf, src)
            want_s[dst] = src_stat[src]
        assert got_p == bytes(want_p) and got_s == bytes(want_s)
        assert d_sp.download() == spts and d_ss.download() == sstat
        # scatter: set point 3 <- point 5, set point 0 <- point 20; a repeated or missing set point, a missing source: refused
        pairs = lambda *v: (ctypes.c_uint32 * len(v))(*v)
        scatter = lambda a, k: N.cg1_chain_scatter_enqueue(ctx.handle, d_p.ptr, d_s.ptr, n_pts, d_sp.ptr, d_ss.ptr, n_set, a, k)
        for bad in ((3, 5, 3, 6), (5, 5, 0, 1), (3, n_pts, 0, 1)):
            assert scatter(pairs(*bad), 2) == N.ERR_ARG, bad
        ctx.check(scatter(pairs(3, 5, 0, 20), 2))
        ctx.check(N.cg1_stream_sync(ctx.handle))
        want_sp, want_ss = bytearray(spts), bytearray(sstat)
        for dst, src in ((3, 5), (0, 20)):
            want_sp[96 * dst: 96 * dst + 96] = rec(got_p, src)
            want_ss[dst] = got_s[src]
        assert d_sp.download() == bytes(want_sp) and d_ss.download() == bytes(want_ss)
        assert d_p.download() == got_p and d_s.download() == got_s
    finally:
        for b in (d_p, d_s, d_sp, d_ss):
            b.free()


# ---------------------------------------------------------------------------------------------------- whole chains
@pytest.mark.parametrize("device_front_end", [False, True])
def test_one_call_of_twelve_blocks_in_three_sub_batches(native_lib, ctx, scenario4, reference_verifier, device_front_end):
    sc = scenario4
    ts, v = chain_verifier(sc.kit, ctx, sc.initial, device_front_end)
    try:
        L, ell = v.crs.points_per_proof, sc.ell
        want = expanded_status(reference_verifier(ell), sc.expanded(sc.blocks))
        assert want == [0] * 12
        got = v.verify_blocks(sc.blocks, rng=random.Random(1))
        assert got == want == v.last_status
        assert ts.trackers() == sc.final.slots and device_set_equals_host(native_lib, ts)
        assert v.last_stats["decoded_points"] == 12 * (L - 2 * ell)          # nothing is decoded twice
        assert v.last_stats["gathered_points"] == 12 * 2 * ell and v.last_stats["valid_prefix"] == 12 and v.last_stats["n"] == 12
        # the wire form, over the same state again
        ts.replace(sc.initial)
        idx = [i for indices, _, _ in sc.blocks for i in indices]
        posts = b"".join(r + k for _, post, _ in sc.blocks for r, k in post)
        proofs = b"".join(proof for _, _, proof in sc.blocks)
        assert v.verify_blocks_packed(idx, posts, proofs, 12) == want and ts.packed() == sc.final.packed()
        # what the caller got wrong raises and leaves the set alone
        for bad in (idx[:-1] + [16], idx[:-1] + [-1], idx[:-1]):
            with pytest.raises(ValueError):
                v.verify_blocks_packed(bad, posts, proofs, 12)
        assert ts.packed() == sc.final.packed() and device_set_equals_host(native_lib, ts)
    finally:
        v.close(); ts.close()


@pytest.mark.parametrize("device_front_end", [False, True])
def test_a_later_call_and_a_later_internal_batch_read_the_resident_set(native_lib, ctx, scenario4, device_front_end):
    sc = scenario4
    ts, v = chain_verifier(sc.kit, ctx, sc.initial, device_front_end)
    try:
        assert v.verify_blocks(sc.blocks[:6]) == [0] * 6 and ts.trackers() == sc.state_after(sc.blocks[:6]).slots
        assert v.verify_blocks(sc.blocks[6:]) == [0] * 6 and ts.trackers() == sc.final.slots
        assert device_set_equals_host(native_lib, ts)
        # twelve internal batches of one block: the verifier's slots rotate while every source lies in the resident set
        ts.replace(sc.initial)
        v.SPLIT = 1
        assert v.verify_blocks(sc.blocks) == [0] * 12
        L, ell = v.crs.points_per_proof, sc.ell
        assert v.last_stats["n"] == 12 and v.last_stats["decoded_points"] == 12 * (L - 2 * ell) and v.last_stats["gathered_points"] == 12 * 2 * ell
        assert ts.trackers() == sc.final.slots and device_set_equals_host(native_lib, ts)
        assert len([b for b in v.verifier._slots if b is not None]) < 12
    finally:
        v.close(); ts.close()


def negated(enc):
    out = bytearray(enc)
    out[0] ^= 0x20
    assert O.g1_decompress(bytes(out)) == O.g1_neg(O.g1_decompress(enc))
    return bytes(out)


@pytest.mark.parametrize("device_front_end", [False, True])
@pytest.mark.parametrize("kind", ["negated", "undecodable"])
def test_a_tampered_post_rejects_writer_and_readers_and_the_set_rolls_back(native_lib, ctx, scenario4, reference_verifier, kind, device_front_end):
    """Block 5 of 12 writes slot 0, which block 7 reads: its r_G replaced by the negated point's encoding, or by one that does not decode."""
    sc = scenario4
    indices, post, proof = sc.blocks[5]
    assert indices[0] == 0 and 0 in sc.blocks[7][0]
    bad_post = [(negated(post[0][0]) if kind == "negated" else bytes(48), post[0][1])] + post[1:]
    blocks = sc.blocks[:5] + [(indices, bad_post, proof)] + sc.blocks[6:]
    want = expanded_status(reference_verifier(sc.ell), sc.expanded(blocks))
    assert want[:5] == [0] * 5 and want[5] != 0 and want[7] != 0 and want[6] == 0
    if kind == "undecodable":
        assert want[5] == want[7] == 2
    ts, v = chain_verifier(sc.kit, ctx, sc.initial, device_front_end)
    try:
        assert v.verify_blocks(blocks, rng=random.Random(1)) == want
        assert v.last_stats["valid_prefix"] == 5
        assert ts.trackers() == sc.state_after(sc.blocks[:5]).slots and device_set_equals_host(native_lib, ts)
        # the untampered rest of the chain was proved over exactly this state
        assert v.verify_blocks(sc.blocks[5:]) == [0] * 7
        assert ts.trackers() == sc.final.slots and device_set_equals_host(native_lib, ts)
    finally:
        v.close(); ts.close()


def test_a_tracker_outside_g1_in_the_set_gets_the_expanded_verdict(native_lib, ctx, scenario4, reference_verifier):
    """Slot 5 of the initial set carries a point on the curve but outside G1 (tests/curve_mul_cases.py offers points, not encodings: the
    encoding is whisk_shuffle_cases.torsion_encoding()).  Block 2 reads it with a proof made for the original tracker."""
    sc = scenario4
    initial = list(sc.initial)
    initial[5] = (W.torsion_encoding(), initial[5][1])
    start = SetModel(initial)
    want = expanded_status(reference_verifier(sc.ell), sc.expanded(sc.blocks[:4], start))
    assert want[:2] == [0, 0] and want[2] != 0 and want[3] == 0
    ts, v = chain_verifier(sc.kit, ctx, initial, None)
    try:
        assert v.verify_blocks(sc.blocks[:4], rng=random.Random(1)) == want
        assert v.last_stats["valid_prefix"] == 2 and ts.trackers() == sc.state_after(sc.blocks[:2], start).slots
        assert device_set_equals_host(native_lib, ts)
    finally:
        v.close(); ts.close()


def test_a_chain_at_ell_12(native_lib, ctx, kits, reference_verifier):
    """Five blocks over 32 slots: sub-batches of two, a block reading its predecessor, a repeated index."""
    sc = Scenario(kits(12), 32, [list(range(12)), list(range(6, 18)), list(range(20, 32)), [0, 0] + list(range(10, 20)), list(range(31, 19, -1))])
    ts, v = chain_verifier(sc.kit, ctx, sc.initial, None, chunk=2)
    try:
        want = expanded_status(reference_verifier(12), sc.expanded(sc.blocks))
        assert want == [0] * 5 and v.verify_blocks(sc.blocks, rng=random.Random(1)) == want
        assert ts.trackers() == sc.final.slots and device_set_equals_host(native_lib, ts)
        assert v.last_stats["decoded_points"] == 5 * (v.crs.points_per_proof - 24)
    finally:
        v.close(); ts.close()


def test_eight_blocks_at_ell_124_over_1024_slots(native_lib, ctx, kits, reference_verifier):
    """Two rounds of four index-disjoint blocks; the second round reads what the first wrote, and untouched slots."""
    ell = 124
    rng = random.Random(124)
    first = [rng.sample(range(r * 200, r * 200 + 200), ell) for r in range(4)]
    second = [rng.sample(first[r] + list(range(800 + 50 * r, 850 + 50 * r)), ell) for r in range(4)]
    sc = Scenario(kits(ell), 1024, first + second)
    ts, v = chain_verifier(sc.kit, ctx, sc.initial, None, chunk=256)
    try:
        want = expanded_status(reference_verifier(ell), sc.expanded(sc.blocks))
        assert want == [0] * 8 and v.verify_blocks(sc.blocks, rng=random.Random(1)) == want
        assert ts.trackers() == sc.final.slots and device_set_equals_host(native_lib, ts)
        assert v.last_stats["decoded_points"] == 8 * (v.crs.points_per_proof - 2 * ell) and v.last_stats["valid_prefix"] == 8
    finally:
        v.close(); ts.close()
