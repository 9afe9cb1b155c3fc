"""The host lineage of a chain of Whisk shuffles proved over a tracker set (cg1_chain_lineage: csrc/chain_lineage.h, exported from
csrc/shuffle_verify.cpp).  No GPU: the entry does no point arithmetic.

Driven at ell = 4 over a set of 8 slots against a Python model of the semantics: block j with permutation pi and secret k reads the
(origin, composite) pairs of its ell slots before any of its own writes, is refused when an origin it reads is flagged (and then writes
nothing), and otherwise writes (origin of slot indices[pi[t]], that slot's composite * k mod r) to slot indices[t], t in order."""
import ctypes
import random

import pytest

from oracle import bls12_381 as O

ELL, SLOTS = 4, 8
NO_DECODE, NOT_G1, NO_ORIGIN = 2, 3, 0xFFFFFFFF


def model(flags, index_lists, perms, ks, n_slots=SLOTS):
    """-> (status, bad_at, origin [n][2][ell], composite [n][2][ell], writers [(slot, b ell + t)] by slot)"""
    cur = {s: (s, 1) for s in range(n_slots)}
    last = {}
    status, bad_at, origin, comp = [], [], [], []
    for b, (idx, pm, k) in enumerate(zip(index_lists, perms, ks)):
        ell = len(idx)
        pre = [cur[i] for i in idx]
        dec = [2 * t + h for t in range(ell) for h in (0, 1) if flags[2 * pre[t][0] + h] == NO_DECODE]
        g1 = [2 * t + h for t in range(ell) for h in (0, 1) if flags[2 * pre[t][0] + h] == NOT_G1]
        if dec or g1:
            status.append(NO_DECODE if dec else NOT_G1)
            bad_at.append(dec[0] if dec else g1[0])
            origin.append([[NO_ORIGIN] * ell] * 2)
            comp.append([[0] * ell] * 2)
            continue
        post = [(pre[pm[t]][0], pre[pm[t]][1] * k % O.R) for t in range(ell)]
        status.append(0)
        bad_at.append(0)
        origin.append([[p[0] for p in pre], [p[0] for p in post]])
        comp.append([[p[1] for p in pre], [p[1] for p in post]])
        for t, i in enumerate(idx):
            cur[i] = post[t]
            last[i] = b * ell + t
    return status, bad_at, origin, comp, sorted(last.items())


def lineage(N, flags, index_lists, perms, ks, n_slots=SLOTS, ell=None, pattern=0xA5):
    """cg1_chain_lineage -> (rc, status, bad_at, origin, composite, writers, untouched): every output buffer is pre-filled with `pattern`
    and `untouched` says whether all of them still hold nothing else"""
    n = len(index_lists)
    ell = (len(index_lists[0]) if n else ELL) if ell is None else ell
    u32 = lambda v: (ctypes.c_uint32 * max(1, len(v)))(*v)
    idx, pm = u32([i for b in index_lists for i in b]), u32([m for p in perms for m in p])
    k32 = b"".join(int(k).to_bytes(32, "little") for k in ks)
    pos = max(1, n * 2 * ell)
    bufs = [ctypes.create_string_buffer(bytes([pattern]) * size, size) for size in (4 * max(1, n), 4 * max(1, n), 4 * pos, 32 * pos, 8 * max(1, min(n_slots, n * ell)))]
    nw = ctypes.c_size_t(12345)
    rc = N.cg1_chain_lineage(n_slots, bytes(flags), idx, pm, k32, n, ell, *bufs, ctypes.byref(nw))
    untouched = all(b.raw == bytes([pattern]) * len(b.raw) for b in bufs) and nw.value == 12345
    if rc:
        return rc, None, None, None, None, None, untouched
    word = lambda raw, i: int.from_bytes(raw[4 * i: 4 * i + 4], "little")
    st = [word(bufs[0].raw, b) for b in range(n)]
    at = [word(bufs[1].raw, b) for b in range(n)]
    origin = [[[word(bufs[2].raw, (b * 2 + w) * ell + t) for t in range(ell)] for w in (0, 1)] for b in range(n)]
    comp = [[[int.from_bytes(bufs[3].raw[32 * ((b * 2 + w) * ell + t): 32 * ((b * 2 + w) * ell + t + 1)], "little") for t in range(ell)] for w in (0, 1)] for b in range(n)]
    writers = [(word(bufs[4].raw, 2 * i), word(bufs[4].raw, 2 * i + 1)) for i in range(nw.value)]
    return rc, st, at, origin, comp, writers, untouched


def draws(seed, n, ell=ELL):
    rng = random.Random(seed)
    perms = [rng.sample(range(ell), ell) for _ in range(n)]
    ks = [rng.randrange(1, O.R) for _ in range(n)]
    return perms, ks


CLEAN = [0] * (2 * SLOTS)
SEQUENCES = {
    "the same indices every time": (CLEAN, [[0, 1, 2, 3]] * 5),
    "overlapping blocks": (CLEAN, [[0, 1, 2, 3], [2, 3, 4, 5], [4, 5, 6, 7], [7, 0, 3, 4], [1, 6, 2, 5]]),
    "an index repeated inside a block": (CLEAN, [[0, 1, 2, 3], [4, 1, 4, 2], [4, 4, 4, 4], [1, 2, 4, 0]]),
    # slot 5's k_r_G does not decode: block 1 is refused and writes nothing, blocks 2 and 3 read slots 4, 6 and 7 as block 0 left them
    "a refused block and its readers": ([0] * 11 + [NO_DECODE] + [0] * 4, [[4, 6, 7, 0], [4, 5, 6, 7], [6, 7, 4, 1], [4, 0, 1, 2], [5, 0, 1, 2]]),
    # slot 1's r_G lies outside G1 (tracker 0) and slot 6's k_r_G does not decode (tracker 3): the decoder's refusal is named first
    "two different flags in one block": ([0, 0, NOT_G1, 0] + [0] * 9 + [NO_DECODE] + [0, 0], [[1, 2, 3, 6], [1, 0, 2, 3], [0, 2, 3, 4]]),
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_lineage_matches_the_model(native_lib, name):
    flags, index_lists = SEQUENCES[name]
    perms, ks = draws(name, len(index_lists))
    rc, st, at, origin, comp, writers, _ = lineage(native_lib, flags, index_lists, perms, ks)
    assert rc == 0
    want = model(flags, index_lists, perms, ks)
    assert (st, at) == (want[0], want[1])
    assert origin == [[list(r) for r in b] for b in want[2]]
    assert comp == [[list(r) for r in b] for b in want[3]]
    assert writers == want[4]


def test_the_refusals_of_the_sequences_are_the_ones_meant(native_lib):
    flags, index_lists = SEQUENCES["a refused block and its readers"]
    perms, ks = draws(1, len(index_lists))
    _, st, at, origin, _, writers, _ = lineage(native_lib, flags, index_lists, perms, ks)
    assert st == [0, NO_DECODE, 0, 0, NO_DECODE] and at[1] == 2 * 1 + 1 and at[4] == 0 * 2 + 1
    assert origin[1] == [[NO_ORIGIN] * ELL] * 2
    assert 5 not in dict(writers)                          # the flagged slot is never written
    assert set(origin[2][0]) <= {0, 1, 4, 6, 7}            # block 2 reads block 0's values (and the untouched slot 1), nothing of block 1's
    flags, index_lists = SEQUENCES["two different flags in one block"]
    perms, ks = draws(2, len(index_lists))
    _, st, at, _, _, _, _ = lineage(native_lib, flags, index_lists, perms, ks)
    assert st == [NO_DECODE, NOT_G1, 0] and at[:2] == [2 * 3 + 1, 0]


def test_composite_times_origin_is_the_step_by_step_product(native_lib):
    """5 blocks over multiples of G: composite * origin == k_j * (... k_1 * origin), point by point, with the oracle"""
    rng = random.Random(21)
    start = [O.g1_mul(O.G1_GEN, rng.randrange(1, O.R)) for _ in range(SLOTS)]
    index_lists = [[0, 1, 2, 3], [2, 3, 4, 5], [2, 3, 4, 5], [5, 0, 7, 2], [3, 3, 1, 0]]
    perms, ks = draws(22, 5)
    ks[2] = O.R - 1
    rc, st, _, origin, comp, writers, _ = lineage(native_lib, CLEAN, index_lists, perms, ks)
    assert rc == 0 and st == [0] * 5
    cur = list(start)
    for b, (idx, pm, k) in enumerate(zip(index_lists, perms, ks)):
        pre = [cur[i] for i in idx]
        post = [O.g1_mul(pre[pm[t]], k) for t in range(ELL)]
        for t in range(ELL):
            assert O.g1_mul(start[origin[b][0][t]], comp[b][0][t]) == pre[t]
            assert O.g1_mul(start[origin[b][1][t]], comp[b][1][t]) == post[t]
        for t, i in enumerate(idx):
            cur[i] = post[t]
    for slot, w in writers:                                # the last writer's post is the slot's final value
        assert O.g1_mul(start[origin[w // ELL][1][w % ELL]], comp[w // ELL][1][w % ELL]) == cur[slot]


@pytest.mark.parametrize("what", ["index >= N", "perm entry >= ell", "no permutation", "k >= r", "ell = 0", "a flag that is no code"])
def test_bad_arguments_are_refused_before_anything_is_written(native_lib, what):
    index_lists = [[0, 1, 2, 3], [4, 5, 6, 7], [0, 2, 4, 6]]
    perms, ks = draws(3, 3)
    flags, ell = list(CLEAN), None
    if what == "index >= N":
        index_lists[2] = [0, 2, SLOTS, 6]
    elif what == "perm entry >= ell":
        perms[1] = [0, 1, 2, ELL]
    elif what == "no permutation":
        perms[2] = [0, 1, 1, 3]
    elif what == "k >= r":
        ks[2] = O.R
    elif what == "ell = 0":
        ell = 0
    else:
        flags[4] = 1
    rc, *_, untouched = lineage(native_lib, flags, index_lists, perms, ks, ell=ell)
    assert rc != 0 and untouched


def test_no_blocks_and_null_outputs(native_lib):
    N = native_lib
    nw = ctypes.c_size_t(7)
    assert N.cg1_chain_lineage(SLOTS, bytes(CLEAN), None, None, None, 0, ELL, None, None, None, None, None, ctypes.byref(nw)) == 0 and nw.value == 0
    idx, pm = (ctypes.c_uint32 * 4)(0, 1, 2, 3), (ctypes.c_uint32 * 4)(3, 2, 1, 0)
    st = (ctypes.c_int32 * 1)(9)
    assert N.cg1_chain_lineage(SLOTS, bytes(CLEAN), idx, pm, (5).to_bytes(32, "little"), 1, ELL, st, None, None, None, None, None) == 0 and st[0] == 0
