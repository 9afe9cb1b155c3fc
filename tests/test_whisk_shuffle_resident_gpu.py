"""Seeded Whisk shuffles proved with the witness resident on the device (ShuffleBatchProver(.., resident_witness=True): the context
parameter "whisk_resident_witness", k_whisk_witness_place in csrc/kernels_whisk_shuffle.h) against the copying path of the same seed,
byte for byte: post trackers, proofs, statuses and refusals.  Needs an MI355X.

The copying path is what tests/test_whisk_shuffle_seeded_gpu.py pins to prove_many and the reference; here only the two paths are held
against each other, at every shape where the placement takes another turn: one prover, a refused prover in the middle (its row of every
column skipped) or at both ends, the 64 provers of a full call, and ell = 4, 12, 60 and 124 (rows of 16 bytes up to the largest).  Then
what the resident path is for: no witness byte crosses to the host (cg1_whisk_last_witness_traffic), and the draws buffer is zero after a
success, after a call refused as a whole and after a growth that failed inside the chain (cg1_whisk_draws_buffer_is_zero)."""
import ctypes
import re
import types

import pytest

import whisk_shuffle_cases as W
import whisk_shuffle_seeded_cases as S
from test_whisk_shuffle_seeded_gpu import Kit, flat

pytestmark = pytest.mark.gpu
NB = S.NB
FRONT, CHAIN = 0, 1


class MadeKit:
    """A CRS and trackers of an ell the fixtures store no points for: multiples of the generator, made by the library."""

    def __init__(self, ell):
        from curdleproofs_pie_amd import G1Point, Scalar
        from curdleproofs_pie_amd.fixed_base import FixedBaseTable
        from curdleproofs_pie_amd.shuffle_prover import ShuffleBatchProver

        n = ell + NB
        pts = [G1Point() * Scalar(0xC0FFEE + 7 * i) for i in range(n + 3)]
        enc = [bytes((G1Point() * Scalar(0x5EED + 11 * i)).to_compressed_bytes()) for i in range(2 * ell)]
        self.ell = ell
        self.crs = types.SimpleNamespace(vec_G=pts[:ell], vec_H=pts[ell:n], H=pts[n], G_t=pts[n + 1], G_u=pts[n + 2])
        self.pre = list(zip(enc[:ell], enc[ell:]))
        self.table = FixedBaseTable(pts)
        self.prover = ShuffleBatchProver(self.crs, table=self.table)

    lists = Kit.lists


@pytest.fixture(scope="module")
def kits(native_lib):
    from curdleproofs_pie_amd.shuffle_prover import ShuffleBatchProver

    made = {}

    def get(ell, fresh=False):
        if fresh or ell not in made:
            kit = Kit(ell) if ell in (4, 12, 28) else MadeKit(ell)
            kit.resident = ShuffleBatchProver(kit.crs, table=kit.table, resident_witness=True)
            made[(ell, len(made)) if fresh else ell] = kit
            return kit
        return made[ell]

    yield get
    for k in made.values():
        k.table.close()


def traffic(N, ctx):
    out = (ctypes.c_uint64 * 2)()
    N.cg1_whisk_last_witness_traffic(ctx.handle, out)
    return int(out[0]), int(out[1])


def field_bytes(N, ell, P, keep, block):
    """the lengths of a block's witness fields, summed (cg1_whisk_witness_block_emulate's list)"""
    nf = ctypes.c_size_t(32)
    fields = (ctypes.c_uint64 * 64)()
    arr = (ctypes.c_size_t * len(keep))(*keep)
    assert N.cg1_whisk_witness_block_emulate(ell, P, arr, len(keep), bytes(64), 1, block, None, 0, fields, ctypes.byref(nf)) > 0
    return sum(int(fields[2 * i + 1]) for i in range(nf.value))


def copying_traffic(N, ell, status):
    """what one native call of the copying path moves of its witness: the draws' staging down; then that staging, the front's fields, the
    gathered rows where a shuffle was refused, vec_a_blinders padded to four, and the chain's fields, written into host memory"""
    P, n = len(status), ell + NB
    keep = [p for p, s in enumerate(status) if not s]
    staging = ((P * ell * 4 + 63) & ~63) + 32 * P * (3 * n + 14)
    written = staging + field_bytes(N, ell, P, list(range(P)), FRONT)
    if keep:
        gathered = len(keep) * (4 * ell + 32 * (3 * n + 14)) if len(keep) < P else 0
        written += gathered + 128 * len(keep) + field_bytes(N, ell, P, keep, CHAIN)
    return staging, written


def no_decode(pre):
    """the list with a tracker the decoder refuses (no compression flag)"""
    return [pre[0], (pre[1][0], b"\x00" * 48)] + pre[2:]


def outside_g1(pre):
    return [pre[0], (W.torsion_encoding(), pre[1][1])] + pre[2:]


def both_ways(N, kit, lists, seed, first_index=0):
    """-> the copying path's (post96, proofs, status), asserted equal to the resident path's, refusals included; the traffic of each"""
    ctx = kit.table._ctx
    want = kit.prover.generate_packed(flat(lists), seed=seed, first_index=first_index)
    want_refusals, copied = list(kit.prover.last_refusals), traffic(N, ctx)
    got = kit.resident.generate_packed(flat(lists), seed=seed, first_index=first_index)
    assert got[2] == want[2] and kit.resident.last_status == kit.prover.last_status and kit.resident.last_refusals == want_refusals
    assert got[0] == want[0] and got[1] == want[1]
    assert traffic(N, ctx) == (0, 0) and N.cg1_whisk_draws_buffer_is_zero(ctx.handle) == 1
    assert copied[0] > 0 and copied[1] > 0 and copied == copying_traffic(N, kit.ell, want[2]), (copied, copying_traffic(N, kit.ell, want[2]))
    return want


SHAPES = [
    ("one", 4, 1, {}),
    ("middle does not decode", 4, 3, {1: no_decode}),
    ("middle outside G1", 4, 3, {1: outside_g1}),
    ("a full call", 4, 64, {}),
    ("first and last refused", 12, 5, {0: outside_g1, 4: no_decode}),
    ("ell = 60", 60, 2, {}),
    ("ell = 124", 124, 2, {}),
]


@pytest.mark.parametrize("name,ell,count,bad", SHAPES, ids=[s[0] for s in SHAPES])
def test_resident_equals_copying(native_lib, kits, name, ell, count, bad):
    N = native_lib
    kit = kits(ell)
    lists = kit.lists(count)
    for p, edit in bad.items():
        lists[p] = edit(lists[p])
    post, proofs, status = both_ways(N, kit, lists, S.SEED_A)
    wb = N.cg1_whisk_shuffle_proof_bytes(ell)
    assert [bool(s) for s in status] == [p in bad for p in range(count)]
    for p in range(count):
        refused = p in bad
        assert (post[96 * ell * p: 96 * ell * (p + 1)] == bytes(96 * ell)) == refused and (proofs[wb * p: wb * (p + 1)] == bytes(wb)) == refused, p
    # item i alone under first_index = i is item i of the batch, in resident mode
    for i in sorted({0, count // 2, count - 1}):
        alone = kit.resident.generate_packed(flat([lists[i]]), seed=S.SEED_A, first_index=i)
        assert alone == (post[96 * ell * i: 96 * ell * (i + 1)], proofs[wb * i: wb * (i + 1)], [status[i]]), i
    assert kit.resident.generate_packed(flat(lists), seed=S.SEED_B)[1] != proofs


def test_all_refused_never_enters_the_chain_and_a_failed_growth_inside_it_wipes_the_draws(native_lib, kits):
    """On a table that has proved nothing: three refused shuffles in resident mode give CG1_OK, their statuses and zeros, and leave the
    table's staging block at the FRONT's length -- so the next call, three valid shuffles with "alloc_fail_at" = 1, meets its first
    growth inside the chain, at the chain's block length: CG1_ERR_HIP, the draws buffer zero, and the same call again gives the copying
    path's bytes."""
    N = native_lib
    kit = kits(4, fresh=True)
    ctx = kit.table._ctx
    ell, count = 4, 3
    wb = N.cg1_whisk_shuffle_proof_bytes(ell)
    lists = kit.lists(count)
    ctx.whisk_shuffle_draws_device(ell, count, S.SEED_B, 0)             # the context's draws buffer holds three shuffles from here on
    bad = [outside_g1(lists[0]), no_decode(lists[1]), outside_g1(lists[2])]
    post, proofs, status = kit.resident.generate_packed(flat(bad), seed=S.SEED_A)
    assert status == [3, 2, 3] and post == bytes(96 * ell * count) and proofs == bytes(wb * count)
    assert kit.resident.last_refusals == [(1, "r_G"), (1, "k_r_G"), (1, "r_G")]
    assert traffic(N, ctx) == (0, 0) and N.cg1_whisk_draws_buffer_is_zero(ctx.handle) == 1
    nf = ctypes.c_size_t(0)
    keep = (ctypes.c_size_t * count)(*range(count))
    length = lambda block: N.cg1_whisk_witness_block_emulate(ell, count, keep, count, bytes(1 << 16), 1, block, None, 0, None, ctypes.byref(nf))
    assert 0 < length(FRONT) < length(CHAIN)
    ctx.set_param("alloc_fail_at", 1)
    try:
        with pytest.raises(N.NativeError, match="injected") as e:
            kit.resident.generate_packed(flat(lists), seed=S.SEED_A)
    finally:
        ctx.set_param("alloc_fail_at", 0)
    assert str(e.value).startswith(f"libcurdle_g1 error {N.ERR_HIP}: "), str(e.value)
    assert int(re.search(r"to (\d+) bytes", str(e.value)).group(1)) == length(CHAIN), str(e.value)
    assert N.cg1_whisk_draws_buffer_is_zero(ctx.handle) == 1
    got = kit.resident.generate_packed(flat(lists), seed=S.SEED_A)
    assert got[2] == [0] * count and N.cg1_whisk_draws_buffer_is_zero(ctx.handle) == 1
    assert got == kit.prover.generate_packed(flat(lists), seed=S.SEED_A)
    # the copying path of the all-refused call: its counters hold the draws' staging and the front's fields, and nothing of the chain
    kit.prover.generate_packed(flat(bad), seed=S.SEED_A)
    n = ell + NB
    staging = ((count * ell * 4 + 63) & ~63) + 32 * count * (3 * n + 14)
    assert traffic(N, ctx) == (staging, staging + count * (32 * n + 4 * ell + 32)) == copying_traffic(N, ell, [3, 2, 3])


def test_a_call_refused_as_a_whole_leaves_the_draws_buffer_zero(native_lib, kits):
    """A CRS index outside the table, in resident mode: CG1_ERR_ARG, the outputs untouched, the draws buffer zero, no traffic; the parameter
    takes 0 and 1 only; and the next call is right."""
    N = native_lib
    kit = kits(4)
    t, ctx = kit.table, kit.table._ctx
    ell, count = 4, 3
    wb = N.cg1_whisk_shuffle_proof_bytes(ell)
    gi, hi, ui, gti, gui, gth = kit.prover._crs_args()
    u32 = lambda v: (ctypes.c_uint32 * len(v))(*v)
    lists = kit.lists(count)
    want = kit.prover.generate_packed(flat(lists), seed=S.SEED_A)
    post, out = ctypes.create_string_buffer(b"\xaa" * (96 * ell * count), 96 * ell * count), ctypes.create_string_buffer(b"\xaa" * (wb * count), wb * count)
    st, at = (ctypes.c_int32 * count)(*([-1] * count)), (ctypes.c_uint32 * count)(*([0xAAAAAAAA] * count))
    with t._ctx_lock():
        for value in (2, -1):
            assert N.cg1_ctx_set_param(ctx.handle, b"whisk_resident_witness", value) == N.ERR_ARG
        ctx.set_param("whisk_resident_witness", 1)
        try:
            rc = N.cg1_whisk_shuffle_prove_seeded(ctx.handle, t._tab.handle, ell, count, u32([0, 1, 2, len(t)] * count), u32(hi * count), u32([ui] * count), u32([gti] * count),
                                                  u32([gui] * count), gth, flat(lists), S.SEED_A, 0, post, out, st, at)
            text = N.cg1_ctx_error(ctx.handle).decode()
            assert rc == N.ERR_ARG and "outside the table" in text and S.SEED_A.hex() not in text
            assert post.raw == b"\xaa" * len(post.raw) and out.raw == b"\xaa" * len(out.raw) and list(st) == [-1] * count
            assert traffic(N, ctx) == (0, 0) and N.cg1_whisk_draws_buffer_is_zero(ctx.handle) == 1
            rc = N.cg1_whisk_shuffle_prove_seeded(ctx.handle, t._tab.handle, ell, count, u32(gi * count), u32(hi * count), u32([ui] * count), u32([gti] * count),
                                                  u32([gui] * count), gth, flat(lists), S.SEED_A, 0, post, out, st, at)
        finally:
            ctx.set_param("whisk_resident_witness", 0)
    assert rc == N.OK and (post.raw, out.raw, list(st)) == want
    assert traffic(N, ctx) == (0, 0) and N.cg1_whisk_draws_buffer_is_zero(ctx.handle) == 1
