"""Every kernel of the MSM's reduction tail -- the chunk folds, the row / column sums, the bit trees, the exports, the device and host
Horners -- on sums that coincide and cancel: the families of tests/msm_tail_cases.py (every bucket equal, alternating signs, mirrored
rows and columns, lone buckets / rows / columns, buckets of 2 .. 18 equal chunks, Horner steps that double and that cancel) through every
switch setting of its configuration list.  Every point is compared byte for byte (compressed) with (sum k_i s_i mod r) G from the Python
oracle, and after every call Context.last_tail() -- which kernels the call really launched -- with == against tail_path, the test's own
statement of msm_enqueue's decision: a switch that stops reaching its kernel fails here.  Nothing has a tolerance.  A wrong point is
localised: the message names the switches, the family, and the windows whose one-window shard differs.

The suspected loss (no fold in front of k_rowcol_quad with fold_quad = 0 and fold_pass = 0): confirmed on the device before the fix.
Against a library without it all 28 cases of test_chunked_buckets failed, each with 12 failures per window the family sits in: a WRONG
point (and no fold in last_tail) under the three settings that put k_rowcol_quad behind no fold (rowcol_row = 0, the same at lgq = 4,
tree_row = 0), whole plan and one-window shard -- and under no other setting.  msm_enqueue now launches k_bucket_fold whenever
k_rowcol_quad is the consumer, and tail_path says so.

Measured on MI355X: the whole file takes 15 s (59 tests); each docstring gives its own share."""
import ctypes

import pytest

import msm_digit_model as M
import msm_tail_cases as T
from curdleproofs_pie_amd import _native as N
from oracle import bls12_381 as O

pytestmark = pytest.mark.gpu
R = T.R
_RAW, _POINT = {0: bytes(96)}, {}


def _raw(k):
    """affine96 of k G from the Python oracle (zeros: the identity), kept."""
    if k not in _RAW:
        p = O.g1_mul(O.G1_GEN, k)
        _RAW[k] = p[0].to_bytes(48, "little") + p[1].to_bytes(48, "little")
    return _RAW[k]


def _expected(log):
    if log not in _POINT:
        _POINT[log] = T.expected_point(log)
    return _POINT[log]


def _compress(blob):
    out = ctypes.create_string_buffer(48)
    N.cg1_compress(out, blob)
    return out.raw


class Dev:
    """A case's terms on the device."""

    def __init__(self, ctx, terms):
        self.n = len(terms)
        self.d_p = ctx.alloc(96 * self.n); self.d_p.upload(b"".join(_raw(k) for _, k in terms))
        self.d_s = ctx.alloc(32 * self.n); self.d_s.upload(b"".join(s.to_bytes(32, "little") for s, _ in terms))

    def free(self):
        self.d_p.free(); self.d_s.free()


class Tail:
    """The file's context: regime A (small_msm = 0) unless a test says otherwise; set() changes only what differs, reset() restores every
    switch this file touches."""

    def __init__(self):
        self.ctx = N.Context(0)
        self.ctx.set_param("small_msm", 0)
        self.cur = dict(T.DEFAULT_PARAMS)
        self.extra = {"small_msm": 0, "chunk_len": 8}

    def set(self, params):
        for k, v in T.DEFAULT_PARAMS.items():
            v = params.get(k, v)
            if self.cur[k] != v:
                self.ctx.set_param(k, v)
                self.cur[k] = v

    def set_extra(self, name, value):
        if self.extra[name] != value:
            self.ctx.set_param(name, value)
            self.extra[name] = value

    def describe(self, n, c, rank=0, world=1, **kw):
        """The planner's word (cg1_msm_call_describe, no GPU) for a call under the switches as they stand."""
        return N.msm_call_describe(dict(self.cur, **self.extra), n, c, rank, world, **kw)["tail"]

    def raw_tail(self):
        return int(N.cg1_get_last_tail(self.ctx.handle))

    def reset(self):
        self.set({})
        self.set_extra("small_msm", 0)
        self.set_extra("chunk_len", 8)


@pytest.fixture(scope="module")
def tail():
    t = Tail()
    yield t
    t.ctx.close()


@pytest.fixture(autouse=True)
def _restore(tail):
    yield
    tail.reset()


def _big(c, p):
    """Plans beyond the default "rowcol_quad_max" (widths 15, 16): the quad leaves run with it raised to the call's bucket count."""
    big = (len(M.plan(c)) << (abs(c) - 1)) > T.DEFAULT_PARAMS["rowcol_quad_max"]
    return dict(p, rowcol_quad_max=-1) if big and "rowcol_quad_max" not in p and p.get("quad", 1) and p.get("rowcol_quad", 1) else p


def _localise(tail, case, dev, c):
    """The windows whose one-window shard differs from the model under the switches as they stand, for a failure message."""
    bad = []
    for w in range(len(case.pl)):
        if case.buckets[w]:
            got = _compress(tail.ctx.msm_device(dev.d_p, dev.d_s, dev.n, window_c=c, shard_rank=w, shard_world=len(case.pl)))
            if got != _expected(case.log([w])):
                lt = tail.ctx.last_tail()
                bad.append(f"window {w} (offset {case.pl[w][0]}, width {case.pl[w][1]}; alone it ran {lt['fold']} / {lt['rowcol']} / {lt['tree']})")
    return "; ".join(bad) or "every one-window shard is right on its own"


def _run(tail, case, dev, c, params, shard, failures):
    """One regime-A call: the point against the oracle, last_tail against the model."""
    nwin = len(case.pl)
    rank, world, windows, nlw = (0, 1, None, nwin) if shard is None else (shard, nwin, [shard], 1)
    p = T.resolve(params, c, nlw)
    tail.set(p)
    got = _compress(tail.ctx.msm_device(dev.d_p, dev.d_s, dev.n, window_c=c, shard_rank=rank, shard_world=world))
    ran = tail.ctx.last_tail()
    want_tail = T.tail_path(c, nlw, dev.n, p, case.e_top(p, windows))
    if ran != want_tail:
        failures.append(f"plan {c}, {params}, shard {shard}, {case.label}: ran {ran}, the model says {want_tail}")
    if tail.raw_tail() != tail.describe(dev.n, c, rank, world, e_top=case.e_top(p, windows)):
        failures.append(f"plan {c}, {params}, shard {shard}, {case.label}: ran {ran}, the planner says {N.decode_tail(tail.describe(dev.n, c, rank, world, e_top=case.e_top(p, windows)))}")
    if got != _expected(case.log(windows)):
        where = _localise(tail, case, dev, c) if shard is None else f"window {shard}"
        failures.append(f"plan {c}, {params}, shard {shard}, {case.label} ({ran['fold']} / {ran['rowcol']} lgq {ran['lgq']} / {ran['tree']} x {ran['tree_waves']} / "
                        f"{ran['export']} / host x {ran['horner_threads']}): WRONG point: {where}")


def _report(failures):
    assert not failures, f"{len(failures)} failures; the first: " + " || ".join(failures[:6])


# ------------------------------------------------------------------ regime A
@pytest.mark.parametrize("c", T.ALL_WIDTHS)
def test_every_leaf_at_every_width(tail, c):
    """Every family in every placement through the list that launches every leaf of the four choices, both sides of "rowcol_quad_max" and
    the one-window shards (2^(cmax - 1) buckets exactly: 8192 at width 14, 16384 at 15, the two sides of the rows' own fold).
    15 plans: 9.9 s -- 0.25 - 0.65 s each up to width 14 (about a thousand calls), 1.3 s at width 15, 2.2 s at 16 and -16 (21 cases of up
    to 32 768 terms through 45 settings over half a million buckets)."""
    failures = []
    todo = [(_big(c, p), s) for p, s in T.configs(c)]
    for case in T.cases(c):
        dev = Dev(tail.ctx, case.terms)
        for params, shard in todo:
            if shard is None or case.w in (None, shard):
                _run(tail, case, dev, c, params, shard, failures)
        dev.free()
    _report(failures)


@pytest.mark.parametrize("c", T.TRIPLE_WIDTHS)
def test_every_legal_triple(tail, c):
    """Every legal (fold, row / column, tree) combination at widths 4, 8 (rows shorter than columns), 9 (equally long) and 14.  4 widths: 0.9 s."""
    failures = []
    for case in T.cases(c, False):
        dev = Dev(tail.ctx, case.terms)
        for params in T.triples():
            _run(tail, case, dev, c, params, None, failures)
        dev.free()
    _report(failures)


CHUNK_VARIANTS = ({}, {"rowcol_row": 0}, {"rowcol_row": 0, "rowcol_lgq": 4}, {"tree_row": 0}, {"rowcol_quad": 0}, {"quad": 0}, {"quad": 0, "tree_row": 0}, {"reduce_2d": 0},
                  {"reduce_2d": 0, "seg_m": 16})


@pytest.mark.parametrize("L0", [1, 2])
@pytest.mark.parametrize("c", [c for c in T.ALL_WIDTHS if T.chunk_cases(c)])
def test_chunked_buckets(tail, c, L0):
    """Buckets of 2, 3, 16, 17 and 18 copies of one point, and of alternating signs, at chunk lengths 1 and 2: every fold setting in front
    of every row / column kernel, whole plan and one-window shard.  fold_quad = 0 with fold_pass = 0 in front of k_rowcol_quad is among
    them: before msm_enqueue folded for that consumer regardless, these calls lost every chunk but the first of each bucket.  28 cases: 2.5 s, 0.13 s at most."""
    failures = []
    tail.set_extra("chunk_len", L0)
    for case in T.chunk_cases(c):
        T.check_family(case, L0)
        dev = Dev(tail.ctx, case.terms)
        assert M.call_chunk_len(L0, dev.n, len(case.pl)) == L0
        for f in T.FOLDS:
            for v in CHUNK_VARIANTS:
                for shard in (None, case.w):
                    _run(tail, case, dev, c, _big(c, dict(f, **v)) if shard is None else dict(f, **v), shard, failures)
        dev.free()
    _report(failures)


def test_host_horner_threads(tail):
    """The host Horner on 1, 2 and 4 threads and with host_split = 0, over calls whose top exported point sits on both sides of bits 96
    and 112: the thread count is the model's and the point is right whichever way the exponent range was cut.  0.07 s."""
    failures = []
    for c, wtop in T.HORNER_TOPS:
        case = T.Case(c, "horner", f"one entry per third window up to {wtop}", T.horner_thread_case(c, wtop), None)
        dev = Dev(tail.ctx, case.terms)
        for params in T.HORNER_THREAD_PARAMS:
            for v in ({}, {"reduce_2d": 0}, {"zero_copy": 0}):
                _run(tail, case, dev, c, dict(params, **v), None, failures)
        dev.free()
    for c in (8, 16, -13):                                     # and with every window full of work for every thread
        case = [x for x in T.cases(c) if x.label == "horner: empty lowest"][0]
        dev = Dev(tail.ctx, case.terms)
        for params in T.HORNER_THREAD_PARAMS:
            _run(tail, case, dev, c, params, None, failures)
        dev.free()
    _report(failures)


# ------------------------------------------------------------------ regime B
@pytest.mark.parametrize("M_,c", [(24, 7), (25, 7), (24, 4), (25, 4), (2048, 4), (2049, 4)])
def test_regime_b_horners(tail, M_, c):
    """M MSMs of 2 .. 4 terms on both sides of the host bound (24) and of the one-wave-per-MSM bound (2048), with horner_row and quad on
    and off and the host bound moved to M and M - 1: the host Horner, k_msm_horner_row, k_msm_horner_quad and k_msm_horner all run, each
    MSM against the oracle.  6 cases: 0.6 s, 0.3 s at most."""
    terms, offs = T.batched_case(c, M_)
    dev = Dev(tail.ctx, terms)
    want = [_expected(sum(k * s for s, k in terms[offs[j]: offs[j + 1]]) % R) for j in range(M_)]
    assert O.g1_compress(None) in want
    failures, ran_kinds = [], set()
    for params in T.batched_params(M_):
        tail.set(params)
        blobs = tail.ctx.msm_batched_device(dev.d_p, dev.d_s, offs, window_c=c)
        ran = tail.ctx.last_tail()
        ran_kinds.add(ran["horner"])
        if ran != T.tail_path_batched(c, M_, params):
            failures.append(f"M {M_}, width {c}, {params}: ran {ran}, the model says {T.tail_path_batched(c, M_, params)}")
        if tail.raw_tail() != tail.describe(dev.n, c, n_msms=M_, max_terms=4):
            failures.append(f"M {M_}, width {c}, {params}: ran {ran}, the planner says another word")
        bad = [j for j, b in enumerate(blobs) if _compress(b) != want[j]]
        if bad:
            failures.append(f"M {M_}, width {c}, {params} ({ran['horner']}): WRONG points of MSMs {bad[:8]} ({len(bad)} in all)")
    dev.free()
    assert ran_kinds == {"host", "k_msm_horner_quad", "k_msm_horner"} | ({"k_msm_horner_row"} if M_ <= T.HORNER_ROW_MAX else set()), ran_kinds
    _report(failures)


# ------------------------------------------------------------------ k_msm_small
def _small_patterns(n):
    """tests/test_msm_small_gpu.py's exceptional bases as terms: one base throughout (doublings inside every chunk), P / -P pairs
    (cancellations), identities in between; under one scalar, a few scalars and spread ones."""
    few = [3, R - 5, (1 << 254) + 7, 0x0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF % R]
    spread = [(0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95 * (i + 1)) % R for i in range(n)]
    return {"same base, same scalar": [(1, T.K)] * n,
            "same base": [(spread[i], T.K) for i in range(n)],
            "plus minus": [(1, T.K if i & 1 else R - T.K) for i in range(n)],
            "plus minus, few scalars": [(few[(i // 2) % 4], T.K if i & 1 else R - T.K) for i in range(n)],
            "plus minus, spread scalars": [(spread[i // 2], T.K if i & 1 else R - T.K) for i in range(n)],
            "identities": [(spread[i], 0 if i % 3 == 0 else (i % 5 + 1) * T.K) for i in range(n)]}


@pytest.mark.parametrize("c", [4, 6, 7, 8, 9])
def test_small_kernel_tails(tail, c):
    """k_msm_small with small_row_tail 1 and 0: the exceptional-base patterns at sizes on both sides of a slice, and the equal, alternating
    and mirror families (at most 1024 terms); three and six MSMs in one launch.  The point, and which tail ran.  5 widths: 0.5 s."""
    failures = []
    tail.set_extra("small_msm", 1)
    todo = [T.Case(c, "small", f"{name}, n = {n}", t, None) for n in (5, 257, 627) for name, t in _small_patterns(n).items()]
    todo += [x for x in T.cases(c) if x.family in ("equal", "alternating", "mirror", "horner") and len(x.terms) <= 1024]
    assert {x.family for x in todo} >= {"small", "equal", "alternating", "horner"}
    for case in todo:
        dev = Dev(tail.ctx, case.terms)
        for rt in (1, 0):
            tail.set({"small_row_tail": rt})
            got = _compress(tail.ctx.msm_device(dev.d_p, dev.d_s, dev.n, window_c=c))
            ran, want_tail = tail.ctx.last_tail(), T.tail_path_small(1, {"small_row_tail": rt}, case.e_top({}))
            if tail.ctx.last_counts()["accumulate_launches"] != 0 or ran != want_tail:
                failures.append(f"width {c}, small_row_tail {rt}, {case.label}: ran {ran}, the model says {want_tail}")
            if tail.raw_tail() != tail.describe(dev.n, c, e_top=case.e_top({})):
                failures.append(f"width {c}, small_row_tail {rt}, {case.label}: ran {ran}, the planner says another word")
            if got != _expected(case.log()):
                failures.append(f"width {c}, small_row_tail {rt}, {case.label}: WRONG point")
        dev.free()
    for M_ in (3, 6):
        terms, offs = T.batched_case(c, M_)
        dev = Dev(tail.ctx, terms)
        for rt in (1, 0):
            tail.set({"small_row_tail": rt})
            blobs = tail.ctx.msm_batched_device(dev.d_p, dev.d_s, offs, window_c=c)
            ran = tail.ctx.last_tail()
            if ran != T.tail_path_small(M_, {"small_row_tail": rt}) or tail.raw_tail() != tail.describe(dev.n, c, n_msms=M_, max_terms=4):
                failures.append(f"width {c}, small_row_tail {rt}, {M_} MSMs: ran {ran}")
            bad = [j for j, b in enumerate(blobs) if _compress(b) != _expected(sum(k * s for s, k in terms[offs[j]: offs[j + 1]]) % R)]
            if bad:
                failures.append(f"width {c}, small_row_tail {rt}, {M_} MSMs in one launch: WRONG points of MSMs {bad}")
        dev.free()
    _report(failures)
