"""A chain of Whisk shuffles PROVED over a device-resident tracker set (curdleproofs_pie_amd/shuffle_chain.py: ShuffleChainProver,
TrackerSet.evolve; csrc/chain_lineage.h, csrc/kernels_chain_prove.h, csrc/capi_chain_prove.h).  Needs an MI355X.

The tracker stage alone first, against the oracle's sequential products at edge scalars.  Then the prover against its DEFINITION: block j's
outputs are item 0 of ShuffleBatchProver.generate_packed(pre_j, seed, first_index + j) over a model of the set kept here, byte for byte in
posts and proofs, and the blocks go through ShuffleChainVerifier over a copy of the initial set.  The CRS and trackers are those of
tests/golden/shuffle_device_vectors.json, as in tests/test_shuffle_chain_gpu.py, whose Kit and SetModel are used here."""
import random

import pytest

from oracle import bls12_381 as O

import codec_edge_cases as E
import whisk_shuffle_cases as W
from test_shuffle_chain_gpu import Kit, SetModel, chain_verifier, device_set_equals_host

pytestmark = pytest.mark.gpu
SEED = bytes(range(100, 132))
NO_DECODE, NOT_G1 = 2, 3


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


def packed(trackers):
    return b"".join(r + k for r, k in trackers)


def pairs(post96, ell):
    return [(post96[96 * i: 96 * i + 48], post96[96 * i + 48: 96 * i + 96]) for i in range(ell)]


def by_definition(kit, model, index_lists, seed=SEED, first_index=0):
    """Block j = item 0 of generate_packed(pre_j, seed, first_index + j) over `model`, which a block with status 0 then advances.
    -> ([(indices, post, proof) or None], statuses, refusals)"""
    blocks, status, refusals = [], [], []
    for j, indices in enumerate(index_lists):
        post96, proof, st = kit.prover.generate_packed(packed(model.read(indices)), seed, first_index=first_index + j)
        status.append(st[0])
        refusals.append(kit.prover.last_refusals[0])
        if st[0]:
            assert post96 == bytes(len(post96)) and proof == bytes(len(proof))
            blocks.append(None)
        else:
            post = pairs(post96, kit.ell)
            model.apply(indices, post)
            blocks.append((list(indices), post, proof))
    return blocks, status, refusals


def chain_prover(kit, ctx, trackers):
    from curdleproofs_pie_amd.shuffle_chain import ShuffleChainProver, TrackerSet

    ts = TrackerSet(trackers, ctx)
    return ts, ShuffleChainProver(kit.crs, ts, table=kit.table)


def verified(kit, ctx, initial, blocks):
    """the blocks through ShuffleChainVerifier over a set of their own -> (statuses, valid prefix, final trackers)"""
    ts, v = chain_verifier(kit, ctx, initial, None)
    try:
        st = v.verify_blocks(blocks, rng=random.Random(1))
        return st, v.last_stats["valid_prefix"], ts.trackers()
    finally:
        v.close(); ts.close()


# 12 blocks at ell = 4 over 12 slots: the same indices three times running (blocks 2, 3, 4), an index repeated inside a block (blocks 5
# and 9), every block but the first reads something an earlier one wrote
DENSE = [[0, 1, 2, 3], [2, 3, 4, 5], [6, 7, 8, 9], [6, 7, 8, 9], [6, 7, 8, 9], [9, 0, 9, 4], [10, 11, 0, 1], [5, 6, 10, 2], [3, 3, 7, 11], [1, 8, 1, 8],
         [11, 10, 9, 0], [4, 5, 6, 7]]


class Dense:
    """the chain DENSE by definition, made once: the initial set, the blocks and the model's final state"""

    def __init__(self, kit):
        self.kit = kit
        self.initial = kit.initial_set(12)
        self.final = SetModel(self.initial)
        self.blocks, self.status, _ = by_definition(kit, self.final, DENSE)
        assert self.status == [0] * len(DENSE)


@pytest.fixture(scope="module")
def dense(kits):
    return Dense(kits(4))


# ---------------------------------------------------------------------------------------------------- 1. the tracker stage alone
def test_evolve_matches_the_oracle_at_edge_scalars(native_lib, ctx, kits):
    """40 dependent blocks over 10 slots, one of which holds the identity: k in {0, 1, 2, r - 1, random}, the identity permutation, a reversal
    and random ones, an index repeated inside a block.  The oracle multiplies step by step."""
    from curdleproofs_pie_amd.shuffle_chain import TrackerSet

    kit, ell, n_slots = kits(4), 4, 10
    rng = random.Random(40)
    initial = kit.initial_set(n_slots)
    initial[3] = (W.INF, W.INF)
    index_lists, perms, ks = [], [], []
    for b in range(40):
        index_lists.append([2, 5, 2, 7] if b == 9 else rng.sample(range(n_slots), ell))
        perms.append([0, 1, 2, 3] if b % 5 == 0 else [3, 2, 1, 0] if b % 5 == 1 else rng.sample(range(ell), ell))
        ks.append({4: 1, 11: 2, 17: O.R - 1, 23: 1, 30: 0, 36: O.R - 1}.get(b, rng.randrange(1, O.R) if b % 3 == 0 else rng.randrange(1, 1 << 16)))
    cur = [(O.g1_decompress(r), O.g1_decompress(k)) for r, k in initial]
    model = SetModel(initial)
    want = []
    for idx, pm, k in zip(index_lists, perms, ks):
        pre = [cur[i] for i in idx]
        post = [(O.g1_mul(pre[pm[t]][0], k), O.g1_mul(pre[pm[t]][1], k)) for t in range(ell)]
        for t, i in enumerate(idx):
            cur[i] = post[t]
        enc = [(O.g1_compress(a), O.g1_compress(b)) for a, b in post]
        model.apply(idx, enc)
        want.append(packed(enc))
    ts = TrackerSet(initial, ctx)
    try:
        post96, status = ts.evolve(index_lists, perms, ks)
        assert status == [0] * 40
        for b in range(40):
            assert post96[96 * ell * b: 96 * ell * (b + 1)] == want[b], f"block {b}: k = {ks[b] if ks[b] < 3 else '...'}, perm {perms[b]}"
        assert ts.trackers() == model.slots
        assert device_set_equals_host(native_lib, ts)
        assert ts.last_evolve_stats["certified_slots"] == n_slots
    finally:
        ts.close()


def test_evolve_refuses_bad_arguments_and_keeps_the_set(native_lib, ctx, kits):
    from curdleproofs_pie_amd.shuffle_chain import TrackerSet

    kit = kits(4)
    initial = kit.initial_set(8)
    ts = TrackerSet(initial, ctx)
    try:
        secret = O.R + 12345
        for args in (([[0, 1, 2, 8]], [[0, 1, 2, 3]], [5]), ([[0, 1, 2, 3]], [[0, 1, 1, 3]], [5]), ([[0, 1, 2, 3]], [[0, 1, 2, 3]], [secret]),
                     ([[0, 1, 2]], [[0, 1, 2, 3]], [5])):
            with pytest.raises(ValueError) as e:
                ts.evolve(*args)
            assert str(secret) not in str(e.value) and hex(secret)[2:] not in str(e.value)
        assert ts.trackers() == initial and device_set_equals_host(native_lib, ts)
    finally:
        ts.close()


# ---------------------------------------------------------------------------------------------------- 2, 3, 5. the definition, the round trip, the cut
def test_prove_blocks_is_generate_packed_block_by_block(native_lib, ctx, dense):
    ts, pr = chain_prover(dense.kit, ctx, dense.initial)
    try:
        got = pr.prove_blocks(DENSE, seed=SEED)
        for j, (g, w) in enumerate(zip(got, dense.blocks)):
            assert g == w, f"block {j}"
        assert pr.last_status == [0] * len(DENSE) and pr.last_refusals == [None] * len(DENSE)
        assert ts.trackers() == dense.final.slots and device_set_equals_host(native_lib, ts)
        assert pr.last_stats["certified_slots"] == 12 and pr.last_stats["native_calls"] == 1
    finally:
        pr.close(); ts.close()


def test_the_proved_blocks_verify_as_a_chain(native_lib, ctx, dense):
    ts, pr = chain_prover(dense.kit, ctx, dense.initial)
    try:
        blocks = pr.prove_blocks(DENSE, seed=SEED)
        st, prefix, final = verified(dense.kit, ctx, dense.initial, blocks)
        assert st == [0] * len(DENSE) and prefix == len(DENSE)
        assert final == ts.trackers() == dense.final.slots
    finally:
        pr.close(); ts.close()


@pytest.mark.parametrize("cut", [1, 5, 11])
def test_the_output_does_not_depend_on_how_a_call_is_cut(native_lib, ctx, dense, cut):
    ts, pr = chain_prover(dense.kit, ctx, dense.initial)
    try:
        head = pr.prove_blocks(DENSE[:cut], seed=SEED)
        tail = pr.prove_blocks(DENSE[cut:], seed=SEED, first_index=cut)
        assert head + tail == dense.blocks
        assert ts.trackers() == dense.final.slots and device_set_equals_host(native_lib, ts)
    finally:
        pr.close(); ts.close()


def test_the_packed_face(native_lib, ctx, dense):
    import numpy as np

    ts, pr = chain_prover(dense.kit, ctx, dense.initial)
    try:
        flat = [i for b in DENSE for i in b]
        post96, proofs, status = pr.prove_blocks_packed(np.asarray(flat, dtype="<u4").tobytes(), len(DENSE), seed=SEED)
        assert status == [0] * len(DENSE)
        assert post96 == b"".join(packed(b[1]) for b in dense.blocks) and proofs == b"".join(b[2] for b in dense.blocks)
        assert pr.prove_blocks_packed([], 0, seed=SEED) == (b"", b"", [])
    finally:
        pr.close(); ts.close()


# ---------------------------------------------------------------------------------------------------- 4. the group boundary
def test_seventy_blocks_cross_the_group_of_64(native_lib, ctx, kits):
    """Blocks 0 .. 63 are one group of the proving chain, 64 .. 69 the next; block 64 reads what 63 wrote, 65 what 62 and 64 wrote.  The
    model is advanced with the prover's own posts up to block 61 (the verifier vouches for them below), and blocks 62 .. 66 are compared
    with the definition."""
    kit, n_slots = kits(4), 16
    rng = random.Random(70)
    index_lists = [rng.sample(range(n_slots), 4) for _ in range(70)]
    index_lists[62], index_lists[63], index_lists[64], index_lists[65] = [0, 1, 2, 3], [4, 5, 6, 7], [7, 6, 8, 9], [1, 8, 2, 10]
    initial = kit.initial_set(n_slots)
    ts, pr = chain_prover(kit, ctx, initial)
    try:
        blocks = pr.prove_blocks(index_lists, seed=SEED)
        assert pr.last_status == [0] * 70
        model = SetModel(initial)
        for indices, post, _ in blocks[:62]:
            model.apply(indices, post)
        want, _, _ = by_definition(kit, model, index_lists[62:67], first_index=62)
        assert blocks[62:67] == want
        st, prefix, final = verified(kit, ctx, initial, blocks)
        assert st == [0] * 70 and prefix == 70 and final == ts.trackers()
        assert device_set_equals_host(native_lib, ts)
    finally:
        pr.close(); ts.close()


# ---------------------------------------------------------------------------------------------------- 6, 7. refusals
def bad_encodings():
    non_square = E.x_range_cases()[2][3][1]
    return E.enc_x(non_square, 0x80), W.torsion_encoding()


def test_blocks_that_read_a_bad_tracker_are_refused_and_write_nothing(native_lib, ctx, kits):
    """Slot 9's r_G does not decode, slot 4's k_r_G lies outside G1.  Blocks 1 and 6 read slot 9, block 3 slot 4, block 5 both (the
    decoder's refusal is named); the others read what their surviving predecessors wrote, and what the refused ones would have."""
    kit = kits(4)
    no_decode, outside = bad_encodings()
    initial = kit.initial_set(12)
    initial[9] = (no_decode, initial[9][1])
    initial[4] = (initial[4][0], outside)
    index_lists = [[0, 1, 2, 3], [1, 9, 2, 5], [1, 2, 5, 6], [6, 4, 0, 7], [6, 0, 7, 8], [11, 4, 9, 0], [9, 9, 9, 9], [8, 5, 11, 10], [3, 2, 1, 0]]
    want_status = [0, NO_DECODE, 0, NOT_G1, 0, NO_DECODE, NO_DECODE, 0, 0]
    want_refusals = [None, (1, "r_G"), None, (1, "k_r_G"), None, (2, "r_G"), (0, "r_G"), None, None]
    ts, pr = chain_prover(kit, ctx, initial)
    ts2, pr2 = chain_prover(kit, ctx, initial)
    try:
        got = pr.prove_blocks(index_lists, seed=SEED)
        assert pr.last_status == want_status and pr.last_refusals == want_refusals
        assert [g is None for g in got] == [s != 0 for s in want_status]
        # ... against generate_packed's verdicts on the same pre trackers
        _, st_def, ref_def = by_definition(kit, SetModel(initial), index_lists)
        assert st_def == want_status and ref_def == want_refusals
        # the list without the refused blocks, every survivor under its own index
        for j, indices in enumerate(index_lists):
            if want_status[j] == 0:
                assert pr2.prove_blocks([indices], seed=SEED, first_index=j) == [got[j]], f"block {j}"
        assert ts.trackers() == ts2.trackers()
        assert ts.trackers()[9] == tuple(initial[9]) and ts.trackers()[4] == tuple(initial[4])
        assert device_set_equals_host(native_lib, ts)
    finally:
        pr.close(); ts.close(); pr2.close(); ts2.close()


def test_refused_blocks_get_zero_bytes_on_the_packed_face(native_lib, ctx, kits):
    kit = kits(4)
    no_decode, _ = bad_encodings()
    initial = kit.initial_set(8)
    initial[2] = (initial[2][0], no_decode)
    ts, pr = chain_prover(kit, ctx, initial)
    try:
        post96, proofs, status = pr.prove_blocks_packed([4, 5, 6, 7, 0, 1, 2, 3], 2, seed=SEED)
        wb = len(proofs) // 2
        assert status == [0, NO_DECODE] and pr.last_refusals == [None, (2, "k_r_G")]
        assert post96[384:] == bytes(384) and proofs[wb:] == bytes(wb) and post96[:384] != bytes(384) and proofs[:wb] != bytes(wb)
    finally:
        pr.close(); ts.close()


def test_certification_is_made_per_call_not_remembered(native_lib, ctx, kits):
    """A first call certifies and writes slot 1; then a tracker outside G1 comes into that slot behind the prover's back (TrackerSet.replace,
    in place of a chain verifier that scattered such a post); the next call that reads it is refused."""
    kit = kits(4)
    _, outside = bad_encodings()
    initial = kit.initial_set(8)
    ts, pr = chain_prover(kit, ctx, initial)
    try:
        assert pr.prove_blocks([[0, 1, 2, 3]], seed=SEED)[0] is not None
        now = [list(t) for t in ts.trackers()]
        now[1][0] = outside
        ts.replace([tuple(t) for t in now])
        before = ts.trackers()
        got = pr.prove_blocks([[4, 5, 6, 7], [3, 1, 0, 2]], seed=SEED, first_index=1)
        assert pr.last_status == [0, NOT_G1] and pr.last_refusals == [None, (1, "r_G")] and got[1] is None
        assert ts.trackers()[:4] == before[:4]
    finally:
        pr.close(); ts.close()


# ---------------------------------------------------------------------------------------------------- 8. errors
def test_caller_errors_raise_before_anything_runs(native_lib, ctx, kits):
    kit = kits(4)
    initial = kit.initial_set(8)
    ts, pr = chain_prover(kit, ctx, initial)
    seed = bytes(range(200, 232))
    try:
        texts = []
        for call in (lambda: pr.prove_blocks([[0, 1, 2, 8]], seed=seed), lambda: pr.prove_blocks([[0, 1, 2, -1]], seed=seed), lambda: pr.prove_blocks([[0, 1, 2]], seed=seed),
                     lambda: pr.prove_blocks_packed([0, 1, 2, 3, 4], 1, seed=seed), lambda: pr.prove_blocks_packed([0, 1, 2, 3], 2, seed=seed),
                     lambda: pr.prove_blocks([[0, 1, 2, 3]], seed=seed, first_index=1 << 32)):
            with pytest.raises(ValueError) as e:
                call()
            texts.append(str(e.value))
        assert ts.trackers() == [tuple(t) for t in initial] and device_set_equals_host(native_lib, ts)
        ts.close()
        with pytest.raises(ValueError) as e:
            pr.prove_blocks([[0, 1, 2, 3]], seed=seed)
        texts.append(str(e.value))
        ts2, _ = chain_prover(kit, ctx, initial)
        pr.set = ts2
        pr.close()
        try:
            with pytest.raises(ValueError) as e:
                pr.prove_blocks([[0, 1, 2, 3]], seed=seed)
            texts.append(str(e.value))
            assert ts2.trackers() == [tuple(t) for t in initial]
        finally:
            ts2.close()
        for t in texts:
            assert seed.hex() not in t and seed.hex()[:16] not in t and repr(seed)[2:18] not in t
    finally:
        ts.close()


# ---------------------------------------------------------------------------------------------------- 9. the consensus size
def test_three_overlapping_blocks_at_ell_124(native_lib, ctx, kits):
    kit, ell = kits(124), 124
    rng = random.Random(124)
    first = rng.sample(range(256), ell)
    second = first[:60] + rng.sample([s for s in range(256) if s not in first[:60]], ell - 60)      # 60 slots of the first block, 64 others
    third = second[30:90] + first[60:124]                                                         # of both, and maybe a slot twice
    index_lists = [first, second, third]
    initial = kit.initial_set(256)
    model = SetModel(initial)
    want, status, _ = by_definition(kit, model, index_lists)
    assert status == [0, 0, 0]
    ts, pr = chain_prover(kit, ctx, initial)
    try:
        got = pr.prove_blocks(index_lists, seed=SEED)
        assert got == want and ts.trackers() == model.slots
        st, prefix, final = verified(kit, ctx, initial, got)
        assert st == [0, 0, 0] and prefix == 3 and final == model.slots
        assert device_set_equals_host(native_lib, ts)
    finally:
        pr.close(); ts.close()
