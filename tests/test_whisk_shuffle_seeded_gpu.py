"""Whisk shuffles proved from a seed (shuffle_prover.ShuffleBatchProver.generate_packed / generate_seeded, cg1_whisk_shuffle_prove_seeded,
cg1_whisk_shuffle_draws_device: csrc/capi_whisk_shuffle.h, csrc/kernels_whisk_shuffle.h).  Needs an MI355X.

The device draws are held against the hashlib model of tests/whisk_shuffle_seeded_cases.py and the host twin; the whole call against
prove_many fed shuffle_draws_from_seed -- which tests/test_whisk_shuffle_prover_gpu.py pins to the reference's bytes -- over the CRS of
the fixture cases of shuffle_device_vectors.json that store their points; every shuffle gets what it gets alone under its own index,
across the cut into native calls; a malformed tracker refuses its own shuffle and no other; and the batch verifier accepts the output."""
import ctypes
import functools
import types

import pytest

from oracle import bls12_381 as O

import whisk_shuffle_cases as W
import whisk_shuffle_seeded_cases as S

pytestmark = pytest.mark.gpu
NB = S.NB


def P(enc):
    from curdleproofs_pie_amd.py_arkworks_bls12381 import G1Point
    return G1Point.from_compressed_bytes_unchecked(enc)


class Kit:
    """A fixture case's CRS as product objects over a FixedBaseTable, a prover over it, and its vec_R / vec_S encodings as trackers."""

    def __init__(self, ell):
        from curdleproofs_pie_amd.fixed_base import FixedBaseTable
        from curdleproofs_pie_amd.shuffle_prover import ShuffleBatchProver

        c = next(c for c in W.golden("shuffle_device_vectors.json") if c["ell"] == ell and "vec_G" in c)
        h = bytes.fromhex
        pts = [P(h(x)) for x in c["vec_G"] + c["vec_H"] + [c["H"], c["G_t"], c["G_u"]]]
        n = ell + NB
        self.ell = ell
        self.crs = types.SimpleNamespace(vec_G=pts[:ell], vec_H=pts[ell:n], H=pts[n], G_t=pts[n + 1], G_u=pts[n + 2])
        self.pre = [(h(r), h(s)) for r, s in zip(c["vec_R"], c["vec_S"])]
        self.table = FixedBaseTable(pts)
        self.prover = ShuffleBatchProver(self.crs, table=self.table)

    def lists(self, count):
        """`count` tracker lists: the fixture's, rotated, the halves exchanged in every other one"""
        out = []
        for i in range(count):
            pre = self.pre[i % self.ell:] + self.pre[: i % self.ell]
            out.append([(s, r) for r, s in pre] if i % 2 else pre)
        return out

    def crs_bytes(self):
        comp = lambda p: bytes(p.to_compressed_bytes())
        add = lambda v: functools.reduce(lambda a, b: a + b, v)
        crs = self.crs
        return b"".join(comp(p) for p in list(crs.vec_G) + list(crs.vec_H) + [crs.H, crs.G_t, crs.G_u, add(crs.vec_G), add(crs.vec_H)])


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


def flat(lists):
    return b"".join(r + s for pre in lists for r, s in pre)


def by_definition(kit, lists, seed, first_index=0):
    """prove_many fed shuffle_draws_from_seed: what generate_packed must return, as flat bytes"""
    from curdleproofs_pie_amd.shuffle_prover import shuffle_draws_from_seed

    got = kit.prover.prove_many([(pre, *shuffle_draws_from_seed(seed, first_index + i, kit.ell)) for i, pre in enumerate(lists)])
    return b"".join(r + s for post, _ in got for r, s in post), b"".join(proof for _, proof in got)


# ---------------------------------------------------------------------------------------------------- the draws
@pytest.mark.parametrize("ell,count", [(4, 1), (4, 3), (4, 64), (12, 5), (124, 2)])
def test_device_draws_equal_the_model_and_the_host_twin(native_lib, kits, ell, count):
    """41 draws per shuffle at ell = 4: shuffles straddle waves and the last block is partial (64 shuffles: 2 624 lanes, 41 blocks)."""
    N = native_lib
    ctx = kits(4).table._ctx
    ns = 3 * (ell + NB) + 14
    for first in (0, (1 << 32) - 64):
        perm, sc = ctx.whisk_shuffle_draws_device(ell, count, S.SEED_A, first)
        assert (perm, sc) == S.columns(S.SEED_A, first, ell, count), (ell, count, first)
        hp, hs = (ctypes.c_uint32 * (ell * count))(), ctypes.create_string_buffer(32 * ns * count)
        assert N.cg1_whisk_shuffle_draws(ell, count, S.SEED_A, first, hp, hs) == N.OK
        assert perm == list(hp) and sc == hs.raw
    assert ctx.whisk_shuffle_draws_device(ell, count, S.SEED_B, 0) == S.columns(S.SEED_B, 0, ell, count)


def test_device_draws_refuse_and_write_nothing(native_lib, kits):
    N = native_lib
    ctx = kits(4).table._ctx
    who = "cg1_whisk_shuffle_draws_device"
    for kw, frag in ((dict(ell=5), "power of two"), (dict(count=N.WHISK_SHUFFLE_DRAWS_MAX_PROVERS + 1), "shuffles"), (dict(first=(1 << 32) - 2), "2^32"),
                     (dict(null="seed"), "bad argument"), (dict(null="perm"), "bad argument"), (dict(null="scalars"), "bad argument")):
        perm = (ctypes.c_uint32 * 12)(*([0xAAAAAAAA] * 12))
        sc = ctypes.create_string_buffer(b"\xaa" * (32 * 38 * 3), 32 * 38 * 3)
        null = kw.get("null")
        rc = N.cg1_whisk_shuffle_draws_device(ctx.handle, kw.get("ell", 4), kw.get("count", 3), None if null == "seed" else S.SEED_A, kw.get("first", 0),
                                              None if null == "perm" else perm, None if null == "scalars" else sc)
        text = N.cg1_ctx_error(ctx.handle).decode()
        assert rc == N.ERR_ARG and text.startswith(who) and frag in text, (kw, text)
        assert all(v == 0xAAAAAAAA for v in perm) and sc.raw == b"\xaa" * len(sc.raw), kw
        assert S.SEED_A.hex() not in text and S.SEED_A not in text.encode()
    assert ctx.whisk_shuffle_draws_device(4, 3, S.SEED_A, 0) == S.columns(S.SEED_A, 0, 4, 3)


# ---------------------------------------------------------------------------------------------------- the whole call
@pytest.mark.parametrize("ell,count", [(4, 1), (4, 3), (12, 3), (28, 2)])
def test_generate_packed_is_prove_many_fed_the_seeded_draws(native_lib, kits, ell, count):
    kit = kits(ell)
    lists = kit.lists(count)
    post, proofs, status = kit.prover.generate_packed(flat(lists), seed=S.SEED_A)
    assert status == [0] * count and kit.prover.last_status == status and kit.prover.last_refusals == [None] * count
    assert len(proofs) == count * native_lib.cg1_whisk_shuffle_proof_bytes(ell) and len(post) == 96 * ell * count
    assert (post, proofs) == by_definition(kit, lists, S.SEED_A)
    assert kit.prover.generate_packed(flat(lists), seed=S.SEED_A) == (post, proofs, status)             # the same seed: the same bytes
    other_post, other_proofs, _ = kit.prover.generate_packed(flat(lists), seed=S.SEED_B)
    wb = len(proofs) // count
    for p in range(count):                                               # another seed: every proof and every post tracker changes
        assert other_proofs[wb * p: wb * (p + 1)] != proofs[wb * p: wb * (p + 1)]
        for i in range(2 * ell):
            at = 96 * ell * p + 48 * i
            assert other_post[at: at + 48] != post[at: at + 48], (p, i)
    if count > 1:                                                        # first_index runs on: the tail of a batch is a batch of its own
        tail = kit.prover.generate_packed(flat(lists[1:]), seed=S.SEED_A, first_index=1)
        assert tail == (post[96 * ell:], proofs[wb:], [0] * (count - 1))


def test_every_shuffle_gets_what_it_gets_alone_across_the_cut(native_lib, kits):
    """70 shuffles at ell = 4 are two native calls (64 + 6); the index runs on across the cut."""
    kit = kits(4)
    ell, lists = 4, kit.lists(70)
    post, proofs, status = kit.prover.generate_packed(flat(lists), seed=S.SEED_B)
    wb = native_lib.cg1_whisk_shuffle_proof_bytes(ell)
    assert status == [0] * 70 and len(proofs) == 70 * wb
    for i in (0, 1, 63, 64, 69):
        alone = kit.prover.generate_packed(flat([lists[i]]), seed=S.SEED_B, first_index=i)
        assert alone == (post[96 * ell * i: 96 * ell * (i + 1)], proofs[wb * i: wb * (i + 1)], [0]), i
    assert (post[: 96 * ell * 2], proofs[: wb * 2]) == by_definition(kit, lists[:2], S.SEED_B)
    assert (post[96 * ell * 69:], proofs[wb * 69:]) == by_definition(kit, lists[69:], S.SEED_B, 69)
    assert len({proofs[wb * i: wb * (i + 1)] for i in range(70)}) == 70


def test_a_bad_tracker_refuses_its_own_shuffle_only(native_lib, kits):
    """A batch of five at ell = 4: item 1 carries, in turn, every tracker refusal of whisk_shuffle_cases.refusals(), item 3 a point outside
    G1.  Status 2 (does not decode: a bad encoding or an x with no point) or 3 (outside G1) for item 1, 3 for item 3, 0 for the others,
    whose bytes equal the clean batch's."""
    N = native_lib
    kit = kits(4)
    ell, lists = 4, kit.lists(5)
    wb = N.cg1_whisk_shuffle_proof_bytes(ell)
    clean = kit.prover.generate_packed(flat(lists), seed=S.SEED_A)
    assert clean[2] == [0] * 5
    item = lambda buf, size, p: buf[size * p: size * (p + 1)]
    torsion = W.torsion_encoding()
    bad3 = [lists[3][0], (torsion, lists[3][1][1])] + lists[3][2:]
    seen = set()
    for name, status_name, edit, fragments in W.refusals():
        if not fragments:
            continue                                                     # (the refusals of k, the blinders and the permutation: nothing a seed can draw)
        bad1 = edit(W.Front("item 1", (), lists[1], list(range(ell)), 1, [0] * NB)).trackers
        code = N.WHISK_SHUFFLE_NOT_G1 if status_name == "ERR_NOT_IN_SUBGROUP" else N.WHISK_SHUFFLE_NO_DECODE
        seen.add(code)
        batch = [lists[0], bad1, lists[2], bad3, lists[4]]
        post, proofs, status = kit.prover.generate_packed(flat(batch), seed=S.SEED_A)
        assert status == [0, code, 0, 3, 0] == kit.prover.last_status, (name, status)
        assert kit.prover.last_refusals == [None, (int(fragments[0].split()[1]), fragments[1]), None, (1, "r_G"), None], (name, kit.prover.last_refusals)
        for p in (1, 3):
            assert item(post, 96 * ell, p) == bytes(96 * ell) and item(proofs, wb, p) == bytes(wb), (name, p)
        for p in (0, 2, 4):
            assert item(post, 96 * ell, p) == item(clean[0], 96 * ell, p) and item(proofs, wb, p) == item(clean[1], wb, p), (name, p)
        got = kit.prover.generate_seeded(batch, seed=S.SEED_A)
        assert got[1] is None and got[3] is None and got[0][1] == item(clean[1], wb, 0) and got[4][1] == item(clean[1], wb, 4)
        assert got[2][0] == [(item(clean[0], 96 * ell, 2)[96 * i: 96 * i + 48], item(clean[0], 96 * ell, 2)[96 * i + 48: 96 * i + 96]) for i in range(ell)]
    assert seen == {2, 3}
    # a decoder refusal wins over an earlier point outside G1, as in the whole-call entries
    both = [(torsion, lists[1][0][1])] + lists[1][1:3] + [(lists[1][3][0], b"\x00" * 48)]
    _, _, status = kit.prover.generate_packed(flat([both]), seed=S.SEED_A)
    assert status == [2] and kit.prover.last_refusals == [(3, "k_r_G")]
    # all refused: statuses only, and the next valid call is right
    post, proofs, status = kit.prover.generate_packed(flat([bad3, both, bad3]), seed=S.SEED_A)
    assert status == [3, 2, 3] and post == bytes(96 * ell * 3) and proofs == bytes(wb * 3)
    assert kit.prover.generate_seeded([bad3, both]) == [None, None]
    assert kit.prover.generate_packed(flat(lists), seed=S.SEED_A) == clean
    assert by_definition(kit, lists[:1], S.SEED_A)[1] == item(clean[1], wb, 0)                          # ... and prove_many after it


def test_a_refused_first_or_last_item_leaves_the_others_their_own_draws(native_lib, kits):
    """Batches of three at ell = 4 with the refused item first, then last: the two survivors move up by one row, or not at all, in every
    column of the witness, and each still gets the proof of prove_many fed the draws of ITS index."""
    N = native_lib
    kit = kits(4)
    ell, lists = 4, kit.lists(3)
    wb = N.cg1_whisk_shuffle_proof_bytes(ell)
    item = lambda buf, size, p: buf[size * p: size * (p + 1)]
    want = [by_definition(kit, [lists[i]], S.SEED_A, i) for i in range(3)]
    for bad in (0, 2):
        batch = list(lists)
        batch[bad] = [lists[bad][0], (W.torsion_encoding(), lists[bad][1][1])] + lists[bad][2:]
        post, proofs, status = kit.prover.generate_packed(flat(batch), seed=S.SEED_A)
        assert status == [3 if p == bad else 0 for p in range(3)], (bad, status)
        for p in range(3):
            if p == bad:
                assert item(post, 96 * ell, p) == bytes(96 * ell) and item(proofs, wb, p) == bytes(wb), (bad, p)
            else:
                assert (item(post, 96 * ell, p), item(proofs, wb, p)) == want[p], (bad, p)


def test_the_batch_verifier_accepts_fresh_seeds(native_lib, kits):
    """Eight shuffles at ell = 28 under seed=None go into are_valid_whisk_shuffle_proofs as they come out; one post tracker replaced by the
    encoding of the negated point (the edit of test_whisk_shuffle_prover_gpu.test_the_batch_verifier_accepts) rejects that item only."""
    from curdleproofs_pie_amd.shuffle_verifier import are_valid_whisk_shuffle_proofs

    kit = kits(28)
    lists = kit.lists(8)
    got = kit.prover.generate_seeded(lists)
    assert kit.prover.last_status == [0] * 8 and all(g is not None for g in got)
    again = kit.prover.generate_seeded(lists)
    assert all(a[1] != b[1] for a, b in zip(got, again))                 # a fresh seed per call
    batch = [(pre, post, proof) for pre, (post, proof) in zip(lists, got)]
    crs = kit.crs_bytes()
    assert are_valid_whisk_shuffle_proofs(crs, batch) == [True] * 8
    pre, post, proof = batch[3]
    r_g = bytearray(post[5][0])
    r_g[0] ^= 0x20
    assert O.g1_decompress(bytes(r_g)) == O.g1_neg(O.g1_decompress(post[5][0]))
    bad = post[:5] + [(bytes(r_g), post[5][1])] + post[6:]
    assert are_valid_whisk_shuffle_proofs(crs, batch[:3] + [(pre, bad, proof)] + batch[4:]) == [True] * 3 + [False] + [True] * 4


def test_inputs_are_not_mutated_and_tracker_objects_are_accepted(native_lib, kits):
    kit = kits(12)
    lists = kit.lists(2)
    objects = [[types.SimpleNamespace(r_G=bytearray(r), k_r_G=bytearray(s)) for r, s in pre] for pre in lists]
    seed = bytearray(S.SEED_A)
    got = kit.prover.generate_seeded(objects, seed=seed, first_index=5)
    assert seed == S.SEED_A and [[(bytes(t.r_G), bytes(t.k_r_G)) for t in pre] for pre in objects] == lists
    assert got == kit.prover.generate_seeded(lists, seed=S.SEED_A, first_index=5)
    post, proofs = by_definition(kit, lists, S.SEED_A, 5)
    assert b"".join(proof for _, proof in got) == proofs and b"".join(r + s for tr, _ in got for r, s in tr) == post


def test_whole_call_refusals_of_the_seeded_entry_leave_every_output_untouched(native_lib, kits):
    """What is not a tracker's fault refuses the call: ERR_ARG under the entry's name, the four outputs as they were, no seed in the text."""
    N = native_lib
    kit = kits(4)
    ell, count = 4, 3
    t = kit.table
    wb = N.cg1_whisk_shuffle_proof_bytes(ell)
    gi, hi, ui, gti, gui, gth = kit.prover._crs_args()
    u32 = lambda v: (ctypes.c_uint32 * max(1, len(v)))(*v)
    trackers96 = flat(kit.lists(count))
    who = "cg1_whisk_shuffle_prove_seeded"

    def call(ell_=ell, count_=count, first=0, g_index=None, null=()):
        post, out = ctypes.create_string_buffer(b"\xaa" * (96 * ell * count), 96 * ell * count), ctypes.create_string_buffer(b"\xaa" * (wb * count), wb * count)
        st, at = (ctypes.c_int32 * count)(*([-1] * count)), (ctypes.c_uint32 * count)(*([0xAAAAAAAA] * count))
        args = dict(tab=t._tab.handle, gi=u32(g_index if g_index is not None else gi * count), hi=u32(hi * count), ui=u32([ui] * count), gti=u32([gti] * count),
                    gui=u32([gui] * count), gth=gth, trackers96=trackers96, seed=S.SEED_A, post=post, out=out, st=st, at=at)
        for key in null:
            args[key] = None
        rc = N.cg1_whisk_shuffle_prove_seeded(t._ctx.handle, args["tab"], ell_, count_, args["gi"], args["hi"], args["ui"], args["gti"], args["gui"], args["gth"],
                                              args["trackers96"], args["seed"], first, args["post"], args["out"], args["st"], args["at"])
        same = post.raw == b"\xaa" * len(post.raw) and out.raw == b"\xaa" * len(out.raw) and list(st) == [-1] * count and list(at) == [0xAAAAAAAA] * count
        return rc, N.cg1_ctx_error(t._ctx.handle).decode(), same, (post.raw, out.raw, list(st))

    with t._ctx_lock():
        for kw, frag in ((dict(ell_=5), "power of two"), (dict(count_=65), "provers"), (dict(first=(1 << 32) - 2), "2^32"), (dict(first=1 << 40), "2^32"),
                         (dict(g_index=[0, 1, 2, len(t)] * count), "outside the table")):
            rc, text, same, _ = call(**kw)
            assert rc == N.ERR_ARG and same and text.startswith(who + ": ") and frag in text, (kw, text)
            assert S.SEED_A.hex() not in text
        for key in ("tab", "gi", "hi", "ui", "gti", "gui", "gth", "trackers96", "seed", "post", "out", "st", "at"):
            rc, text, same, _ = call(null=(key,))
            assert rc == N.ERR_ARG and same and "bad argument" in text, key
        rc, text, same, (post, out, st) = call()                         # the next valid call is right
    assert rc == N.OK and not same and st == [0] * count
    assert (post, out) == kit.prover.generate_packed(trackers96, seed=S.SEED_A)[:2]
