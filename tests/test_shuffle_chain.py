"""cg1_chain_expand (csrc/shuffle_verify.cpp): the host half of a chain of Whisk shuffles over one tracker set -- blocks of (indices, post
trackers) expanded to the verifier's instances, the source plan of every pre position, the last writer of every slot and the updated set,
against a model of the set kept here (no product code).  No GPU: the function only moves bytes, so the trackers are random bytes."""
import ctypes
import random

import pytest

STRIDE_EXTRA = 89          # a proof's own points behind its 4 ell tracker points: L = 4 ell + 89


class SetModel:
    """The tracker set of a chain: block j reads [set[i] for i in indices_j] before any of its writes, then writes post_j[t] to
    indices_j[t] for t = 0 .. ell - 1 in order."""

    def __init__(self, trackers):
        self.slots = [(bytes(r), bytes(k)) for r, k in trackers]
        self.writer = {}                                   # slot -> (block, t) of its last write

    def apply(self, block, indices, post):
        pre = [self.slots[i] for i in indices]
        for t, (i, p) in enumerate(zip(indices, post)):
            self.slots[i] = (bytes(p[0]), bytes(p[1]))
            self.writer[i] = (block, t)
        return pre

    def packed(self):
        return b"".join(r + k for r, k in self.slots)


def expand(N, set96, n_slots, indices, posts96, n, ell, stride, want=("inst", "plan", "writers"), call_ell=None):
    """-> rc, set bytes after, instances, plan list, writer pairs; buffers pre-filled with 0xAA so that untouched outputs show"""
    buf = ctypes.create_string_buffer(set96, len(set96))
    idx = (ctypes.c_uint32 * max(1, len(indices)))(*indices)
    inst = ctypes.create_string_buffer(b"\xaa" * (n * 4 * ell * 48), n * 4 * ell * 48)
    plan = (ctypes.c_int32 * (n * 2 * ell))(*([-0x55555556] * (n * 2 * ell)))
    cap = min(n_slots, n * ell)
    wr = (ctypes.c_uint32 * (2 * cap))(*([0xAAAAAAAA] * (2 * cap)))
    nw = ctypes.c_size_t(0xAAAA)
    rc = N.cg1_chain_expand(buf, n_slots, idx, posts96, n, ell if call_ell is None else call_ell, stride, inst if "inst" in want else None, plan if "plan" in want else None,
                            wr if "writers" in want else None, ctypes.byref(nw) if "writers" in want else None)
    return rc, buf.raw, inst.raw, list(plan), list(wr), nw.value


def random_chain(rng, n_slots, ell, n_blocks):
    """Blocks over a small set: slots are rewritten many times; every third block repeats an index; block 0 and the blocks that draw from
    the slots kept aside read only untouched slots."""
    tracker = lambda: (rng.randbytes(48), rng.randbytes(48))
    trackers = [tracker() for _ in range(n_slots)]
    untouched = list(range(n_slots - ell, n_slots))        # written by nobody but the blocks that read only them
    blocks = []
    for b in range(n_blocks):
        if b == 7:
            indices = list(untouched)                      # reads only slots nobody has written
        else:
            indices = [rng.randrange(n_slots - ell) for _ in range(ell)]
            if b % 3 == 2:
                indices[ell - 1] = indices[0]              # a duplicate inside the block
        blocks.append((indices, [tracker() for _ in range(ell)]))
    return trackers, blocks


@pytest.mark.parametrize("n_slots", [8, 16])
def test_expand_equals_the_model(native_lib, n_slots):
    N = native_lib
    ell, n = 4, 50
    stride = 4 * ell + STRIDE_EXTRA
    rng = random.Random(1000 + n_slots)
    trackers, blocks = random_chain(rng, n_slots, ell, n)
    model = SetModel(trackers)
    before = model.packed()
    want_inst = []
    for b, (indices, post) in enumerate(blocks):
        pre = model.apply(b, indices, post)
        want_inst.append(b"".join(r for r, _ in pre) + b"".join(k for _, k in pre) + b"".join(r for r, _ in post) + b"".join(k for _, k in post))
    flat_idx = [i for indices, _ in blocks for i in indices]
    posts96 = b"".join(r + k for _, post in blocks for r, k in post)
    rc, after, inst, plan, wr, nw = expand(N, before, n_slots, flat_idx, posts96, n, ell, stride)
    assert rc == N.OK
    assert inst == b"".join(want_inst)
    assert after == model.packed()
    want_wr = [(s, b * ell + t) for s, (b, t) in sorted(model.writer.items())]
    assert nw == len(want_wr) and [(wr[2 * j], wr[2 * j + 1]) for j in range(nw)] == want_wr
    assert any(len(set(indices)) < ell for indices, _ in blocks) and max(sum(i == s for ix, _ in blocks for i in ix) for s in range(n_slots)) >= 3
    # every plan entry names a record whose wire bytes are the expanded pre encoding: a post position of an EARLIER block, or the set as it was
    from_set = from_batch = 0
    for b in range(n):
        for p in range(2 * ell):
            v = plan[b * 2 * ell + p]
            want = inst[(b * 4 * ell + p) * 48: (b * 4 * ell + p + 1) * 48]
            if v >= 0:
                sb, sp = divmod(v, stride)
                assert sb < b and 2 * ell <= sp < 4 * ell, (b, p, v)
                assert inst[(sb * 4 * ell + sp) * 48: (sb * 4 * ell + sp + 1) * 48] == want, (b, p, v)
                assert (sp < 3 * ell) == (p < ell)                                    # r_G from a T position, k_r_G from a U position
                from_batch += 1
            else:
                assert 0 <= ~v < 2 * n_slots and (~v & 1) == (p >= ell), (b, p, v)
                assert before[48 * ~v: 48 * ~v + 48] == want, (b, p, v)
                from_set += 1
    assert from_set >= 2 * ell and from_batch > from_set
    assert all(v < 0 for v in plan[7 * 2 * ell: 8 * 2 * ell]) and all(v < 0 for v in plan[: 2 * ell])      # blocks reading only untouched slots
    # the outputs are optional one by one, and a prefix of the blocks gives the state after that prefix (the rollback's replay)
    rc, after2, inst2, plan2, wr2, _ = expand(N, before, n_slots, flat_idx, posts96, n, ell, stride, want=())
    assert rc == N.OK and after2 == after and inst2 == b"\xaa" * len(inst2) and set(plan2) == {-0x55555556}
    prefix = SetModel(trackers)
    for b, (indices, post) in enumerate(blocks[:17]):
        prefix.apply(b, indices, post)
    assert expand(N, before, n_slots, flat_idx, posts96, 17, ell, stride, want=())[1] == prefix.packed()
    assert expand(N, before, n_slots, flat_idx, posts96, 0, ell, stride)[:2] == (N.OK, before)


def test_refusals_leave_every_output_untouched(native_lib):
    N = native_lib
    ell, n, n_slots = 4, 6, 8
    stride = 4 * ell + STRIDE_EXTRA
    rng = random.Random(7)
    trackers, blocks = random_chain(rng, n_slots, ell, n)
    before = SetModel(trackers).packed()
    posts96 = b"".join(r + k for _, post in blocks for r, k in post)
    good = [i for indices, _ in blocks for i in indices]

    def untouched(res):
        rc, after, inst, plan, wr, nw = res
        return (rc == N.ERR_ARG and after == before and inst == b"\xaa" * len(inst) and set(plan) == {-0x55555556} and set(wr) == {0xAAAAAAAA}
                and nw == 0xAAAA)

    for at in (0, ell * n - 1, 9):                                       # an index >= N, in the first block, the last and in between
        for bad_index in (n_slots, 0xFFFFFFFF):
            bad = list(good)
            bad[at] = bad_index
            assert untouched(expand(N, before, n_slots, bad, posts96, n, ell, stride)), (at, bad_index)
    assert untouched(expand(N, before, n_slots, good, posts96, n, ell, stride, call_ell=0))
    assert untouched(expand(N, before, n_slots, good, posts96, n, ell, 4 * ell - 1))     # a stride that cannot hold the tracker points
    assert untouched(expand(N, before, n_slots, good, None, n, ell, stride))             # no posts
    assert expand(N, before, n_slots, good, posts96, n, ell, stride)[0] == N.OK          # the next valid call is right
