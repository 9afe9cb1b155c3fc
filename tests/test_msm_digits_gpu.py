"""The digit recoding, the bucket sort and the chunk plan of the MSM engine on the device, pinned to the integer model of
tests/msm_digit_model.py: the directed families (tie digit in every window, most negative digit, carry chains, carry-only top window,
both signs of both halves of the split) through every plan of regime A, the other recoder and the sort's variants, window shards, the
endomorphism split, the single-launch kernel and regime B, chosen loads in chosen buckets at every edge of the chunk plan, and a refused
call.  Every point is compared byte for byte (compressed) with (sum k_i s_i mod r) G from the Python oracle, every counter of
cg1_get_last_counts with == against the model; nothing here has a tolerance.  A mismatch is localised: the message names the plan, and
the windows whose one-window shard differs from the model.

What the engines report (read from kernels_small.h and the regime-B chain): regime A and regime B report the model's entries and
chunks (regime B's buckets are per MSM); k_msm_small reports the model's entries and 0 chunks -- it cuts its buckets into chunks of 4
inside the workgroup and exports no chunk count.

Measured on MI355X: the whole file takes 6.6 s (61 tests); each docstring gives its own share."""
import ctypes
import functools
import random

import pytest

import msm_digit_model as M
from curdleproofs_pie_amd import _native as N
from oracle import bls12_381 as O
from oracle import c_oracle as C

pytestmark = pytest.mark.gpu
R = M.R
GEN96 = O.G1_GEN[0].to_bytes(48, "little") + O.G1_GEN[1].to_bytes(48, "little")
DEFAULTS = {"partition_sort": 1, "scan_one": 1, "stage_sort": 1, "wave_agg": 1, "host_split": 1, "sort_sub_bits": 0, "reduce_2d": 1, "quad": 1,
            "chunk_len": 8, "chunk_rule": 1, "small_msm": 1, "glv": 0}


# ------------------------------------------------------------------ bases and expected points
@functools.lru_cache(maxsize=None)
def _pool():
    """16 multiples k_j G from the Python oracle, one of them twice -> (k_j, their affine96 records)."""
    rng = random.Random(0xD161)
    ks = [rng.randrange(1, R) for _ in range(16)]
    ks[11] = ks[2]                                         # the duplicated base
    raw = []
    for k in ks:
        p = O.g1_mul(O.G1_GEN, k)
        raw.append(p[0].to_bytes(48, "little") + p[1].to_bytes(48, "little"))
    return ks, raw


@functools.lru_cache(maxsize=64)
def _bases(n, thirds=False, plain=False):
    """-> (k_i with 0 for an identity record, the n affine96 records): the pool in turn, an identity record at i = 5 mod 23 (none with
    `plain`), and with `thirds` one at every third index as well."""
    ks, raw = _pool()
    coef = [0 if ((i % 23 == 5 and not plain) or (thirds and i % 3 == 0)) else ks[i % 16] for i in range(n)]
    return coef, b"".join(bytes(96) if k == 0 else raw[i % 16] for i, k in enumerate(coef))


def _expected(coef, values):
    """compress((sum k_i v_i mod r) G) by the Python oracle."""
    tot = sum(k * v for k, v in zip(coef, values)) % R
    return O.g1_compress(O.g1_mul(O.G1_GEN, tot)) if tot else O.g1_compress(None)


def _compress(blob):
    out = ctypes.create_string_buffer(48)
    N.cg1_compress(out, blob)
    return out.raw


def _s32(scalars):
    return b"".join(s.to_bytes(32, "little") for s in scalars)


class Call:
    """One set of inputs on the device; run() -> (compressed point, entries, chunks)."""

    def __init__(self, ctx, scalars, p96):
        self.ctx, self.n = ctx, len(scalars)
        self.d_p = ctx.alloc(96 * self.n); self.d_p.upload(p96)
        self.d_s = ctx.alloc(32 * self.n); self.d_s.upload(_s32(scalars))

    def run(self, c, rank=0, world=1):
        blob = self.ctx.msm_device(self.d_p, self.d_s, self.n, window_c=c, shard_rank=rank, shard_world=world)
        lc = self.ctx.last_counts()
        return _compress(blob), lc["entries"], lc["chunks"]


def _localise(call, c, scalars, coef, glv, L0, rows):
    """The windows whose one-window shard (rank w of nwin) differs from the model, for a failure message."""
    pl = M.plan(c, glv)
    ident = [k == 0 for k in coef]
    bad = []
    for w in range(len(pl)):
        got = call.run(c, w, len(pl))
        e, ch = M.counts(scalars, ident, pl, glv, w, len(pl), L0, rows=rows)
        want = (_expected(coef, [M.shard_value(s, pl, glv, [w]) for s in scalars]), e, ch)
        if got != want:
            bad.append(f"window {w} (offset {pl[w][0]}, width {pl[w][1]}): point {'ok' if got[0] == want[0] else 'WRONG'}, entries {got[1]} / {want[1]}, chunks {got[2]} / {want[2]}")
    return "; ".join(bad) or "every one-window shard agrees with the model"


def _check(ctx, c, scalars, coef, p96, L0, glv=False, rows=None, rank=0, world=1):
    """One regime-A call against the model -> (entries, chunks)."""
    pl = M.plan(c, glv)
    own = M.owned(len(pl), rank, world)
    nrows = (2 if glv else 1) * len(scalars)
    L = M.call_chunk_len(L0, nrows, len(own), world)
    assert L == L0, (c, L0, L)
    assert N.msm_call_describe({"small_msm": 0, "chunk_len": L0, "glv": 2 if glv else 0}, len(scalars), c, rank, world)["chunk_len"] == L      # the planner's own answer
    if rows is None:
        rows = [M.rows_of(s, pl, glv) for s in scalars]
    ident = [k == 0 for k in coef]
    e, ch = M.counts(scalars, ident, pl, glv, rank, world, L, rows=rows)
    values = scalars if world == 1 else [M.shard_value(s, pl, glv, own) for s in scalars]
    want = (_expected(coef, values), e, ch)
    call = Call(ctx, scalars, p96)
    got = call.run(c, rank, world)
    assert ctx.timings()["window_c"] == c, (c, ctx.timings()["window_c"])
    if got != want:
        where = _localise(call, c, scalars, coef, glv, L0, rows) if world == 1 else ""
        raise AssertionError(f"plan {c} (split {glv}, chunk_len {L0}, shard {rank}/{world}): point {'ok' if got[0] == want[0] else 'WRONG'}, "
                             f"entries {got[1]} / model {want[1]}, chunks {got[2]} / model {want[2]}: {where}")
    return e, ch


@pytest.fixture(scope="module")
def ctx():
    """One context for the file, on the regime-A chain (small_msm = 0) unless a test says otherwise; every test restores what it sets."""
    c = N.Context(0)
    c.set_param("small_msm", 0)
    yield c
    c.close()


def _restore(ctx, names):
    for k in names:
        ctx.set_param(k, 0 if k == "small_msm" else DEFAULTS[k])


# ------------------------------------------------------------------ a. regime A, every plan
@pytest.mark.parametrize("c", M.WIDTHS)
def test_regime_a_every_plan(ctx, c):
    """The plan's family in one call, at chunk lengths 8 and 1, then with every third base an identity: window_c, the point and both
    counters; the identities take exactly their own digits out of the entries.  26 plans: 0.7 s, 0.02 - 0.11 s each."""
    pl = M.plan(c)
    fam = list(M.edge_scalars(c))
    rows = [M.rows_of(s, pl, False) for s in fam]
    try:
        for L0 in (8, 1):
            ctx.set_param("chunk_len", L0)
            coef, p96 = _bases(len(fam))
            e_all, _ = _check(ctx, c, fam, coef, p96, L0, rows=rows)
            coef3, p96_3 = _bases(len(fam), True)
            e_third, _ = _check(ctx, c, fam, coef3, p96_3, L0, rows=rows)
            gone = sum(1 for i, r in enumerate(rows) if coef[i] and not coef3[i] for d in r[0] if d)
            assert gone > 0 and e_all - e_third == gone, (c, L0)
    finally:
        _restore(ctx, ["chunk_len"])


# ------------------------------------------------------------------ b. the other recoder and the sort's variants
@pytest.mark.parametrize("c", [5, 13, -15, 16])
def test_sort_variants_agree_with_the_default_path(ctx, c):
    """k_hist / k_scatter (partition_sort = 0: the recoder of the path above 2^23 terms), the three-launch scans, the sort without its LDS
    stage and without wave aggregation, every sub-bucket width, the 1-D reduction and the tails without quads: the same point and the
    same counters as the default path, which equals the model.  sort_sub_bits = 1 is outside the parameter's range (4 .. 8) and must be
    refused, leaving the width as it was.  4 plans: 0.2 s."""
    fam = list(M.edge_scalars(c))
    coef, p96 = _bases(len(fam))
    want = _check(ctx, c, fam, coef, p96, 8)
    variants = [{"partition_sort": 0}, {"scan_one": 0}, {"stage_sort": 0}, {"wave_agg": 0}, {"host_split": 0}, {"sort_sub_bits": 4}, {"sort_sub_bits": 8},
                {"reduce_2d": 0}, {"quad": 0}]
    with pytest.raises(N.NativeError):
        ctx.set_param("sort_sub_bits", 1)
    assert _check(ctx, c, fam, coef, p96, 8) == want
    for params in variants:
        try:
            for k, v in params.items():
                ctx.set_param(k, v)
            assert _check(ctx, c, fam, coef, p96, 8) == want, (c, params)
        finally:
            _restore(ctx, params)


# ------------------------------------------------------------------ c. window shards
@pytest.mark.parametrize("c", [9, 16, -13])
@pytest.mark.parametrize("world", [2, 3, 5])
def test_window_shards(ctx, c, world):
    """Every rank's counters and partial point are the model's for its windows w = rank (mod world); the partials add up to the whole
    MSM; a rank beyond the window count has nothing: 0 entries, 0 chunks, the identity.  9 cases: 0.15 s."""
    pl = M.plan(c)
    fam = list(M.edge_scalars(c))
    rows = [M.rows_of(s, pl, False) for s in fam]
    coef, p96 = _bases(len(fam))
    total = None
    call = Call(ctx, fam, p96)
    for rank in range(world):
        _check(ctx, c, fam, coef, p96, 8, rows=rows, rank=rank, world=world)
        out = ctypes.create_string_buffer(96)
        N.cg1_to_affine96(out, ctx.msm_device(call.d_p, call.d_s, call.n, window_c=c, shard_rank=rank, shard_world=world))
        total = out.raw if total is None else C.add(total, out.raw)
    assert C.compress(total) == _expected(coef, fam), (c, world)
    nwin = len(pl)
    assert call.run(c, nwin, nwin + 1) == (O.g1_compress(None), 0, 0), c       # (after calls that did count something)


# ------------------------------------------------------------------ d. the endomorphism split
@pytest.mark.parametrize("c", [8, 11, 14, 16, -13, -14])
def test_split_families(ctx, c):
    """glv = 2 over pool points (multiples of G: the promise the parameter makes holds): the point, and the counters over the 2n rows of
    the 128-position plan -- row n + i with term i's identity flag; then the same scalars without the split against the 256-position
    model.  6 plans: 0.4 s."""
    fam = list(M.edge_scalars_glv(c))
    coef, p96 = _bases(len(fam))
    try:
        ctx.set_param("glv", 2)
        _check(ctx, c, fam, coef, p96, 8, glv=True)
        ctx.set_param("glv", 0)
        _check(ctx, c, fam, coef, p96, 8)
    finally:
        _restore(ctx, ["glv"])


# ------------------------------------------------------------------ e. the single-launch kernel and regime B
def _ragged_offsets(n, m, seed):
    rng = random.Random(seed)
    cuts = sorted(rng.randrange(n + 1) for _ in range(m - 1))
    cuts[3] = cuts[2]                                      # an empty MSM
    return [0] + cuts + [n]


@pytest.mark.parametrize("c", [4, 6, 7, 8, 9])
def test_small_kernel_and_regime_b(ctx, c):
    """The family through k_msm_small (default switches, calls of <= 1 024 terms: accumulate_launches == 0) and as 70 ragged MSMs of one
    regime-B call.  k_msm_small reports the model's entries and no chunks; regime B the model's entries and chunks with buckets per MSM.
    5 widths: 0.5 s."""
    pl = M.plan(c)
    fam = list(M.edge_scalars(c))
    coef, p96 = _bases(len(fam))
    ident = [k == 0 for k in coef]
    try:
        ctx.set_param("small_msm", 1)
        for lo in range(0, len(fam), 1024):
            sc, cf = fam[lo: lo + 1024], coef[lo: lo + 1024]
            got = Call(ctx, sc, p96[96 * lo: 96 * (lo + 1024)]).run(c)
            assert ctx.last_counts()["accumulate_launches"] == 0 and ctx.timings()["window_c"] == c
            assert got == (_expected(cf, sc), M.counts(sc, ident[lo: lo + 1024], pl)[0], 0), (c, lo)
        offs = _ragged_offsets(len(fam), 70, c)
        call = Call(ctx, fam, p96)
        blobs = ctx.msm_batched_device(call.d_p, call.d_s, offs, window_c=c)
        lc = ctx.last_counts()
        assert ctx.timings()["window_c"] == c
        assert (lc["entries"], lc["chunks"]) == M.counts(fam, ident, pl, L0=8, offsets=offs), c
        for j, blob in enumerate(blobs):
            lo, hi = offs[j], offs[j + 1]
            assert _compress(blob) == _expected(coef[lo:hi], fam[lo:hi]), (c, j, lo, hi)
    finally:
        ctx.set_param("small_msm", 0)


@pytest.mark.parametrize("c", [4, 9])
def test_every_family_scalar_as_its_own_msm(ctx, c):
    """M = family size one-term MSMs in one regime-B call, each against the CPU oracle's scalar multiplication: a scalar the recoder gets
    wrong is named by its index and value.  2 widths: 0.3 s."""
    fam = list(M.edge_scalars(c))
    _, raw = _pool()
    p96 = b"".join(raw[j % 16] for j in range(len(fam)))
    call = Call(ctx, fam, p96)
    blobs = ctx.msm_batched_device(call.d_p, call.d_s, list(range(len(fam) + 1)), window_c=c)
    lc = ctx.last_counts()
    assert (lc["entries"], lc["chunks"]) == M.counts(fam, [False] * len(fam), M.plan(c), L0=8, offsets=list(range(len(fam) + 1)))
    bad = [(j, hex(s)) for j, (s, blob) in enumerate(zip(fam, blobs)) if _compress(blob) != C.compress(C.scalar_mul(raw[j % 16], s.to_bytes(32, "little")))]
    assert not bad, (c, bad[:8])


# ------------------------------------------------------------------ f. chosen loads in chosen buckets
def _load_call(ctx, c, L0, sc, rank=0, world=1, plain=False):
    """One bucket-load call -> what it returned.  Where the call is large enough for "chunk_rule" to lengthen the chunks (2^20 rows x
    windows: the two loads at the 4096-chunk edge with chunk_len = 8 in the 32 windows of c = 8) the rule is switched off for the call,
    so that the bucket sits on the edge it was built for."""
    coef, p96 = _bases(len(sc), False, plain)
    nlw = len(M.owned(len(M.plan(c)), rank, world))
    rule = M.call_chunk_len(L0, len(sc), nlw, world) == L0
    assert M.call_chunk_len(L0, len(sc), nlw, world, chunk_rule=rule) == L0
    if rule:
        return _check(ctx, c, sc, coef, p96, L0, rank=rank, world=world)
    try:
        ctx.set_param("chunk_rule", 0)
        want = (_expected(coef, sc),) + M.counts(sc, [k == 0 for k in coef], M.plan(c), L0=L0)
        got = Call(ctx, sc, p96).run(c)
        assert got == want, (c, L0, "chunk_rule 0", got[1:], want[1:], got[0] == want[0])
        return want[1:]
    finally:
        _restore(ctx, ["chunk_rule"])


@pytest.mark.parametrize("c", [8, 16, -13])
@pytest.mark.parametrize("L0", [1, 8])
def test_bucket_loads(ctx, c, L0):
    """1, L0 - 1, L0, L0 + 1, 2 L0, 16 L0 (the last bucket k_bucket_fold folds), 16 L0 + 1 and 17 L0 (k_heavy_combine), 4096 L0 and
    4096 L0 + 1 (longer chunks) entries in bucket 1, the tie bucket and two neighbours across a bin edge of the first, a middle and the top
    window; one call with folded (2, 16 chunks) and combined (17 chunks) buckets side by side; then the call that fills the heavy list to the bound it is sized from.  The 4096 L0 + 1 load and the heavy-list call run a
    second time after an unrelated small call: the one memset that clears the chunk-length histogram, the fold flags and the heavy
    list leaves nothing behind.  6 cases: 3.8 s -- 0.2 s each at chunk length 1, 0.9 - 1.2 s at 8, where nine calls of 32 768 terms are built on the host."""
    small = list(M.edge_scalars(c))[:40]
    try:
        ctx.set_param("chunk_len", L0)
        for label, sc in M.bucket_load_cases(c, L0):
            first = _load_call(ctx, c, L0, sc)
            if label.startswith(f"load {4096 * L0 + 1},"):
                _check(ctx, c, small, *_bases(len(small)), L0)
                assert _load_call(ctx, c, L0, sc) == first, (c, L0, label)
        _load_call(ctx, c, L0, M.mixed_load_case(c, L0))      # folded and combined buckets in one call
        world = {8: 3, 16: 2, -13: 2}[c] if L0 == 1 else 1
        sc, own = M.heavy_list_case(c, L0, world)
        first = _load_call(ctx, c, L0, sc, 0, world, plain=True)      # (no identity record: every bucket keeps its 16 L0 + 1 entries)
        assert first[1] == 17 * len(own) * (len(sc) // (16 * L0 + 1))          # every bucket heavy: 17 chunks each
        _check(ctx, c, small, *_bases(len(small)), L0)
        assert _load_call(ctx, c, L0, sc, 0, world, plain=True) == first
    finally:
        _restore(ctx, ["chunk_len"])


# ------------------------------------------------------------------ g. refusals stay clean
@pytest.mark.parametrize("c,small", [(16, 0), (-13, 0), (8, 1)])
def test_a_refused_scalar_leaves_the_context_clean(ctx, c, small):
    """One scalar of the family replaced by 2^255: the call is refused with the encoding error, and the next call on the same context
    returns the right point and counters (regime A, and k_msm_small, whose bad-scalar word lives in counters kept between calls).
    3 cases: under 0.1 s."""
    pl = M.plan(c)
    fam = list(M.edge_scalars(c))[:600]
    coef, p96 = _bases(len(fam))
    bad = list(fam)
    bad[len(bad) // 2] = 1 << 255
    try:
        ctx.set_param("small_msm", small)
        with pytest.raises(N.NativeError, match="2\\^255"):
            Call(ctx, bad, p96).run(c)
        e, ch = M.counts(fam, [k == 0 for k in coef], pl, L0=8)
        assert Call(ctx, fam, p96).run(c) == (_expected(coef, fam), e, 0 if small else ch), c
    finally:
        ctx.set_param("small_msm", 0)
