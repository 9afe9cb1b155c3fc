"""tests/msm_tail_cases.py checked on the host: the families have the properties that force doublings and cancellations in any correct
reduction tail, their closed forms are what the oracle's compute_MSM gives, and the configuration list reaches every leaf of every choice
the tail makes, with a call on each side of every threshold; and the engine's own planner (cg1_msm_call_describe: which engine serves a
call, its plan, its tail word) against these models and against expectations written out here.  No GPU."""
import pytest

import msm_digit_model as M
import msm_tail_cases as T
from curdleproofs_pie_amd import _native as N
from oracle import bls12_381 as O

R = T.R


@pytest.mark.parametrize("c", T.ALL_WIDTHS)
def test_families_have_their_properties(c):
    """cases() asserts each family's property from the digit model when it builds it (check_family); here: every family is present in the
    first, a middle and the top window, each case's exported points add up to its own point under the 2-D and every 1-D item layout, and
    the chunks family has buckets of exactly 16, 17 and 18 chunks at chunk length 1 and folded ones at 2."""
    cs = T.cases(c)
    fams = {x.family for x in cs}
    assert {"equal", "alternating", "mirror", "sparse", "horner"} <= fams, (c, fams)
    for name in ("equal", "alternating") if abs(c) <= 10 else ("alternating",):
        assert {x.w for x in cs if x.family == name} == set(T.placements(c)), (c, name)
    for x in cs:
        for params in ({}, {"reduce_2d": 0, "seg_m": 1}, {"reduce_2d": 0, "seg_m": 4}, {"reduce_2d": 0, "seg_m": 16}):
            assert 0 <= x.e_top(params) < 256
    assert any(x.log() == 0 for x in cs) and any(x.log() != 0 for x in cs), c         # closed forms that are deliberately the identity, too
    for x in T.chunk_cases(c):
        for L0 in (1, 2):
            T.check_family(x, L0)


@pytest.mark.parametrize("c", [4, 5, 6, -5])
def test_closed_forms_are_the_oracles_msm(c):
    """At the smallest widths every case's closed form (sum k s mod r) G, whole and per one-window shard, is what compute_MSM gives over
    the case's own points and scalars -- the identity included."""
    pts = {}
    for x in T.cases(c) + T.chunk_cases(c):
        bases = [pts.setdefault(k, O.g1_mul(O.G1_GEN, k)) for _, k in x.terms]
        got = O.compute_MSM(bases, [s for s, _ in x.terms])
        assert O.g1_compress(got) == T.expected_point(x.log()), (c, x.label)
        if x.w is not None:
            assert x.log([x.w]) == x.log(), (c, x.label)
    zero = [x for x in T.cases(c) if x.log() == 0]
    assert zero and all(T.expected_point(x.log()) == O.g1_compress(None) for x in zero)


def _all_paths():
    """Every regime-A tail the configuration list asks for -> [(c, params, shard, path)]."""
    out = []
    for c in T.ALL_WIDTHS:
        nwin = len(M.plan(c))
        todo = T.configs(c) + ([(p, None) for p in T.triples()] if c in T.TRIPLE_WIDTHS else [])
        for params, shard in todo:
            nlw = nwin if shard is None else 1
            p = T.resolve(params, c, nlw)
            out.append((c, p, shard, T.tail_path(c, nlw, 1 << (abs(c) - 1), p, 0)))
    return out


def test_the_configurations_reach_every_leaf_at_every_width():
    """Every leaf of the four choices at every width 4 .. 16 and the balanced plans -13 and -16."""
    paths = _all_paths()
    for c in T.ALL_WIDTHS:
        mine = [t for cc, _, _, t in paths if cc == c]
        assert {t["fold"] for t in mine} == {None, "k_bucket_fold_quad", "k_bucket_fold"}, c
        assert {t["rowcol"] for t in mine} == {"k_rowcol_quad_row", "k_rowcol_quad", "k_rowcol", "k_seg_reduce"}, c
        assert {t["lgq"] for t in mine if t["rowcol"] == "k_rowcol_quad"} == {2, 3, 4}, c
        assert {t["rowcol_use_quad"] for t in mine if t["rowcol"] == "k_rowcol"} == {0, 1}, c
        assert {t["seg_m"] for t in mine if t["rowcol"] == "k_seg_reduce"} == {min(m, 1 << (abs(c) - 1)) for m in (1, 2, 4, 8, 16)}, c
        assert {t["tree"] for t in mine} == {None, "k_small_tree_row", "k_small_tree_quad", "k_small_tree"}, c
        assert len({t["tree_waves"] for t in mine if t["tree"] == "k_small_tree_quad"}) >= (2 if T.geometry(c)[1] >= 5 else 1), c      # (a block is 64 threads at least)
        assert {t["export"] for t in mine} == {"k_small_tree_row", "k_export_host", "hipMemcpyAsync"}, c
        for tree in ("k_small_tree_row", "k_small_tree_quad", "k_small_tree"):                 # zero_copy 0 and 1 under each tree kernel
            assert len({t["export"] for t in mine if t["tree"] == tree}) == 2, (c, tree)
        # no fold at all only where the consumer adds the chunk sums itself
        assert all(t["rowcol"] != "k_rowcol_quad" for t in mine if t["fold"] is None), c
    waves = {t["tree_waves"] for _, _, _, t in paths if t["tree"] == "k_small_tree_row"}
    assert waves == {1, 2, 4, 8, 16, 32} & waves and {1, 2, 4, 8, 16} <= waves
    assert {t["tree_waves"] for _, _, _, t in paths if t["tree"] == "k_small_tree_quad"} == {1, 2, 4, 8}
    geo = {T.geometry(c)[1:] for c in T.ALL_WIDTHS}
    assert (2, 1) in geo and (8, 7) in geo                      # (lb, hb) from (2, 1) to (8, 7): rows shorter than 2^lgq quads do occur


def test_every_legal_triple_at_the_product_widths():
    """(fold, row / column, tree) at widths 4, 8, 9 and 14: everything the switches can make."""
    for c in T.TRIPLE_WIDTHS:
        nwin = len(M.plan(c))
        got = set()
        for params in T.triples():
            t = T.tail_path(c, nwin, 1, params)
            got.add((t["fold"], t["rowcol"], t["lgq"], t["rowcol_use_quad"], t["tree"]))
        legal = set()
        rows_fold = (nwin << (c - 1)) <= T.ROWS_FOLD_MAX
        for f in (None, "k_bucket_fold_quad", "k_bucket_fold"):
            if f is None or not rows_fold:                         # up to 8192 buckets the rows fold for themselves: nothing else is launched
                legal.add((f, "k_rowcol_quad_row", 0, 0, "k_small_tree_row"))
            if f is not None:                                      # k_rowcol_quad always has a fold in front
                legal |= {(f, "k_rowcol_quad", q, 0, tr) for q in (2, 3, 4) for tr in ("k_small_tree_row", "k_small_tree_quad")}
            legal.add((f, "k_seg_reduce", 0, 0, None))
            if f != "k_bucket_fold_quad":                          # the quad fold belongs to the quad row / column kernels
                legal |= {(f, "k_rowcol", 0, 1, tr) for tr in ("k_small_tree_row", "k_small_tree_quad")}
                legal |= {(f, "k_rowcol", 0, 0, tr) for tr in ("k_small_tree_row", "k_small_tree")}
        assert got == legal, (c, sorted(map(str, got ^ legal)))
    assert T.geometry(8)[1] != T.geometry(8)[2] and T.geometry(9)[1] == T.geometry(9)[2]      # R != Cn at 8, R == Cn at 9


def test_every_threshold_has_a_call_on_each_side():
    """8192 buckets (the rows' own fold), "rowcol_quad_max" at the call's bucket count and one less, bits 96 and 112 of the host Horner,
    24 and 2048 MSMs of regime B and the moved host bound."""
    paths = _all_paths()
    nb = lambda c, shard: (1 if shard is not None else len(M.plan(c))) << (abs(c) - 1)
    rowq = [(nb(c, s), t) for c, p, s, t in paths if t["rowcol"] == "k_rowcol_quad_row"]
    assert any(n == 8192 and t["fold"] is None for n, t in rowq) and any(n == 16384 and t["fold"] == "k_bucket_fold_quad" for n, t in rowq)
    assert any(n == 16384 and t["fold"] == "k_bucket_fold" for n, t in rowq) and any(n == 16384 and t["fold"] is None for n, t in rowq)
    for c in T.ALL_WIDTHS:
        for shard in (None, len(M.plan(c)) // 2):
            quads = lambda p: p.get("reduce_2d", 1) and p.get("quad", 1) and p.get("rowcol_quad", 1)
            at = [t for cc, p, s, t in paths if cc == c and s == shard and quads(p) and p.get("rowcol_quad_max") == nb(c, shard)]
            below = [t for cc, p, s, t in paths if cc == c and s == shard and quads(p) and p.get("rowcol_quad_max") == nb(c, shard) - 1]
            assert at and all(t["rowcol"] in ("k_rowcol_quad_row", "k_rowcol_quad") for t in at), (c, shard)
            assert below and all(t["rowcol"] == "k_rowcol" for t in below), (c, shard)
    tops = sorted({M.plan(c)[w][0] for c, w in T.HORNER_TOPS})
    assert any(e < 96 for e in tops) and 96 in tops and any(96 < e < 112 for e in tops) and 112 in tops and any(e > 112 for e in tops)
    for c, w in T.HORNER_TOPS:
        case = T.Case(c, "horner", "threads", T.horner_thread_case(c, w), None)
        e = case.e_top({})
        assert e == M.plan(c)[w][0]
        got = {(p["horner_threads"], p["host_split"]): T.tail_path(c, len(M.plan(c)), 1, p, e)["horner_threads"] for p in T.HORNER_THREAD_PARAMS}
        assert got[(4, 1)] == (1 if e < 96 else 2 if e < 112 else 4) and got[(2, 1)] == got[(1, 1)] == (1 if e < 96 else 2), (c, w, got)
        assert got[(4, 0)] == got[(2, 0)] == got[(1, 0)] == 1
    kinds = {}
    for M_ in T.BATCHED_M:
        for p in T.batched_params(M_):
            kinds.setdefault(T.tail_path_batched(7, M_, p)["horner"], set()).add(M_)
    assert kinds["host"] >= {24, 25, 2048, 2049} and kinds["k_msm_horner_row"] >= {25, 2048} and 2049 not in kinds["k_msm_horner_row"]
    assert kinds["k_msm_horner_quad"] >= {25, 2048, 2049} and kinds["k_msm_horner"] >= {25, 2048, 2049}
    assert T.tail_path_batched(7, 24, {})["horner"] == "host" and T.tail_path_batched(7, 25, {})["horner"] == "k_msm_horner_row"
    assert T.tail_path_batched(7, 2049, {})["horner"] == "k_msm_horner_quad"
    assert {T.tail_path_small(1, {"small_row_tail": v})["small_row_tail"] for v in (0, 1)} == {0, 1}


def test_the_suspected_combination_is_in_the_list():
    """fold_quad = 0 and fold_pass = 0 in front of k_rowcol_quad, whole plan and one-window shard, at every width -- and the model says a
    fold runs there all the same (msm_enqueue launches k_bucket_fold whenever k_rowcol_quad is the consumer)."""
    for c in T.ALL_WIDTHS:
        hit = [(p, s) for p, s in T.configs(c) if not p.get("fold_quad", 1) and not p.get("fold_pass", 1)
               and T.tail_path(c, 1 if s is not None else len(M.plan(c)), 1, T.resolve(p, c, 1 if s is not None else len(M.plan(c))))["rowcol"] == "k_rowcol_quad"]
        assert {s is None for _, s in hit} == {True, False}, c
        for p, s in hit:
            nlw = 1 if s is not None else len(M.plan(c))
            assert T.tail_path(c, nlw, 1, T.resolve(p, c, nlw))["fold"] == "k_bucket_fold", (c, p)
    assert any(p == T.SUSPECT for p, _ in T.configs(8))
    for x in T.chunk_cases(8):                                     # and the chunks family gives it buckets of 2 .. 16 chunks to lose
        assert any(2 <= M.chunk_count(cnt, 1) < T.HEAVY for _, cnt in x.buckets[x.w].values())


# ------------------------------------------------------------------ the engine's planner (cg1_msm_call_describe) against the models
REGIME_A = {"small_msm": 0, "chunk_len": 8}                        # what tests/test_msm_tail_gpu.py's context runs under


def _described_tail(params, n, c, shard=None, e_top=0, **kw):
    rank, world = (0, 1) if shard is None else (shard, len(M.plan(c)))
    d = N.msm_call_describe(dict(T.DEFAULT_PARAMS, **params), n, c, rank, world, e_top=e_top, **kw)
    return N.decode_tail(d["tail"])


def test_the_planner_takes_every_regime_a_path_the_model_takes():
    """Every configuration of the list (every leaf at every width, both sides of "rowcol_quad_max", the one-window shards, every legal
    triple at the product widths): the planner's tail word, decoded, == tail_path."""
    paths = _all_paths()
    assert len(paths) > 700
    for c, p, shard, want in paths:
        assert _described_tail(dict(p, **REGIME_A), 1 << (abs(c) - 1), c, shard) == want, (c, p, shard)


def test_the_planner_counts_the_host_horners_threads_as_the_model_does():
    for c, w in T.HORNER_TOPS:
        n, e = len(T.horner_thread_case(c, w)), M.plan(c)[w][0]
        for p in T.HORNER_THREAD_PARAMS:
            for v in ({}, {"reduce_2d": 0}, {"zero_copy": 0}):
                q = dict(p, **v)
                assert _described_tail(dict(q, **REGIME_A), n, c, e_top=e) == T.tail_path(c, len(M.plan(c)), n, q, e), (c, w, q)


def test_the_planner_takes_every_regime_b_and_small_path_the_model_takes():
    for M_ in T.BATCHED_M:
        for c in (4, 7):
            for p in T.batched_params(M_):
                got = _described_tail(dict(p, **REGIME_A), 3 * M_, c, n_msms=M_, max_terms=4)
                assert got == T.tail_path_batched(c, M_, p), (M_, c, p)
    for rt in (0, 1):
        p = {"small_row_tail": rt}
        for e in (0, 95, 96, 111, 112, 254):
            for ht in T.HORNER_THREAD_PARAMS:
                q = dict(p, **ht)
                assert _described_tail(q, 627, 7, e_top=e) == T.tail_path_small(1, q, e), (q, e)                      # cg1_msm_device
                assert _described_tail(q, 627, 7, e_top=e, n_msms=1, max_terms=627) == T.tail_path_small(1, q, e)     # one MSM, batched
        for M_ in (4, 5, 64):
            assert _described_tail(p, 3 * M_, 7, n_msms=M_, max_terms=4, e_top=200) == T.tail_path_small(M_, p), (M_, rt)


def _route(switches, n, c=0, rank=0, world=1, **kw):
    d = N.msm_call_describe(switches, n, c, rank, world, **kw)
    return None if d is None else (d["engine"], d["c"], d["glv"])


def test_routing_on_each_side_of_every_threshold():
    """Who serves a call, the plan's width and whether the endomorphism split is on: written out, not computed."""
    A, A2, B, B2, SMALL = "regime A", "regime A, two chains", "regime B", "regime B, two chains", "k_msm_small"
    assert _route({}, 0) == (None, 0, False) and _route({}, 1) == (SMALL, 4, False)
    # SM_MAX_N = 2048 terms: 32 windows x 8 slices is one round of workgroups
    assert _route({}, 2048) == (SMALL, 8, False) and _route({}, 2049) == (A, 8, False)
    assert _route({"small_msm": 0}, 2048) == (A, 8, False) and _route({}, 2048, world=2) == (A, 8, False)
    assert _route({}, 1536, c=7) == (SMALL, 7, False) and _route({}, 1537, c=7) == (A, 7, False)      # 37 windows x 6 slices = 222 workgroups, x 7 = 259: more than one round of 256
    assert _route({}, 1536) == (SMALL, 7, False) and _route({}, 1537) == (SMALL, 8, False)
    assert _route({}, 627, c=5) == (A, 5, False) and _route({}, 627, c=10) == (A, 10, False) and _route({}, 627, c=9) == (SMALL, 9, False)
    # "glv" = 1: the single launch over 2n entries up to 1024 terms, regime A's split up to "glv_max_n" = 2^14 terms
    G = {"glv": 1}
    assert _route(G, 1024) == (SMALL, 8, True) and _route(G, 1025) == (SMALL, 7, False)
    assert _route(G, 2049) == (A, 8, True)
    assert _route(G, 1 << 14) == (A, -13, True) and _route(G, (1 << 14) + 1) == (A, -13, False)
    assert _route(G, 1 << 14, source_kind=2) == (A, -12, False)       # a resident vector holds n records: no split
    assert _route(dict(G, partition_sort=0), 1 << 14) == (A, -12, False)
    assert _route({"glv": 2}, 1 << 22) == (A, 16, True) and _route({"glv": 2}, (1 << 22) + 1) == (A, 16, False)      # 2n <= 2^23
    assert _route(dict(G, glv_max_n=1 << 15), 1 << 15) == (A, -13, True) and _route(dict(G, glv_max_n=1 << 15), (1 << 15) + 1) == (A, -13, False)
    # the automatic plan
    for n, c in ((128, 4), (129, 8), (8192, 8), (8193, -12), (1 << 14, -12), ((1 << 14) + 1, -13), (3 << 15, -13), ((3 << 15) + 1, -15),
                 (3 << 16, -15), ((3 << 16) + 1, 16), (1 << 20, 16)):
        assert _route({"small_msm": 0}, n) == (A, c, False), n
    assert _route({"auto_plan": 0}, 1 << 14) == (A, 16, False) and _route({"auto_plan": 0}, 8192) == (A, 8, False)
    # "split": from "split_min_log2n" terms on, where the rank owns two windows at least
    S = {"split": 1}
    assert _route(S, (1 << 17) - 1, c=16) == (A, 16, False) and _route(S, 1 << 17, c=16) == (A2, 16, False)
    assert _route(S, 1 << 17, c=16, rank=0, world=16) == (A, 16, False) and _route(S, 1 << 17, c=16, rank=0, world=8) == (A2, 16, False)
    assert _route(S, 1 << 17, c=16, rank=15, world=15) is None and _route(S, 1 << 17, c=16, rank=14, world=15) == (A, 16, False)
    assert _route(dict(S, split_min_log2n=10), 1023, c=16) == (A, 16, False) and _route(dict(S, split_min_log2n=10), 1024, c=16, world=2) == (A2, 16, False)
    # regime B: "batched_split_min_m"
    b = lambda sw, M_, c=0, per=4: _route(sw, per * M_, c, n_msms=M_, max_terms=per)
    assert b({"batched_split": 1}, 255, 7) == (B, 7, False) and b({"batched_split": 1}, 256, 7) == (B2, 7, False) and b({}, 256, 7) == (B, 7, False)
    assert b({"batched_split": 1, "batched_split_min_m": 2}, 2, 7, per=4096) == (B2, 7, False)
    assert b({"glv": 1}, 256, 7) == (B, 7, True)
    # one k_msm_small launch: SM_MAX_MSMS = 64 MSMs, SM_MAX_GROUPS = 2560 workgroups (windows x slices x MSMs), SM_MAX_N terms each
    assert b({}, 64, 7) == (SMALL, 7, False) and b({}, 65, 7) == (B, 7, False)
    assert b({}, 40, 4) == (SMALL, 4, False) and b({}, 41, 4) == (B, 4, False)                          # 64 windows: 2560 / 2624
    assert b({}, 34, 7, per=257) == (SMALL, 7, False) and b({}, 35, 7, per=256) == (SMALL, 7, False)    # 37 windows x 2 slices x 34 = 2516; x 35 = 2590
    assert b({}, 35, 7, per=257) == (B, 7, False) and b({}, 1, 8, per=2048) == (SMALL, 8, False) and b({}, 1, 8, per=2049) == (B, 8, False)
    assert b({"small_msm": 0}, 4, 7) == (B, 7, False) and b({}, 4, 5) == (B, 5, False) and b({}, 0) == (None, 0, False)
    # the refusals
    for c in (3, 17, -3, -17):
        assert _route({}, 2049, c) is None and _route({}, 5, c) is None, c
    assert _route({}, 2049, 4) == (A, 4, False) and _route({}, 2049, -16) == (A, -16, False)
    assert b({}, 100, 10) is None and b({}, 100, 3) is None and b({}, 100, 9) == (B, 9, False)
    assert _route({}, 1 << 31) is None and _route({"small_msm": 0}, (1 << 31) - 1, 16) == (A, 16, False)
    assert b({}, 65536) is None and _route({}, 1 << 31, n_msms=4, max_terms=1 << 29) is None
    for rank, world in ((1, 1), (2, 2), (-1, 1), (0, 0), (0, 256)):
        assert _route({}, 2049, 8, rank, world) is None, (rank, world)
    assert _route({}, 2049, 8, 254, 255) == (A, 8, False)
    assert _route({}, 5, source_kind=3) is None and _route({}, 5, source_kind=-1) is None


# (name, lowest, highest) of every MSM switch with a range of values; the others store value != 0
SWITCH_RANGES = (("chunk_len", 1, 65536), ("glv", 0, 2), ("glv_max_n", 0, 2**31 - 1), ("rowcol_quad_max", 0, 2**31 - 1), ("batched_host_horner_max", 0, 2**31 - 1),
                 ("batched_split_min_m", 2, 2**31 - 1), ("tree_shift", -1, 4), ("profile", 0, 2), ("split_min_log2n", 10, 31))
SWITCH_SETS = (("seg_m", (1, 2, 4, 8, 16)), ("horner_threads", (1, 2, 4)), ("rowcol_lgq", (0, 2, 3, 4)), ("sort_sub_bits", (0, 4, 5, 6, 7, 8)))
SWITCH_FLAGS = ("chunk_rule", "stage_sort", "quad", "reduce_2d", "partition_sort", "big_bins", "scan_one", "fold_pass", "fold_quad", "rowcol_quad", "rowcol_row",
                "tree_row", "tree_half", "zero_copy", "host_split", "arm_helpers", "horner_row", "small_msm", "small_row_tail", "auto_plan", "split",
                "batched_split", "blocking_sync")


def test_every_switch_accepts_its_range_and_nothing_beyond():
    ok = lambda name, v: N.msm_call_describe({name: v}, 5) is not None
    assert len(SWITCH_RANGES) + len(SWITCH_SETS) + len(SWITCH_FLAGS) == 36
    for name, lo, hi in SWITCH_RANGES:
        assert ok(name, lo) and ok(name, hi) and not ok(name, lo - 1), name
        assert hi == 2**31 - 1 or not ok(name, hi + 1), name
    for name, values in SWITCH_SETS:
        for v in range(min(values) - 1, max(values) + 2):
            assert ok(name, v) == (v in values), (name, v)
    for name in SWITCH_FLAGS:
        assert all(ok(name, v) for v in (0, 1, -1, 7)), name
    for name in ("", "nonsense", "chunk_len ", "L0", "use_partition_sort", "split_min_n", "merlin_lanes", "alloc_fail_at", "wave_agg"):
        assert not ok(name, 1), name
    # a setting that is refused refuses the call, wherever it stands; a later setting of a name wins
    assert N.msm_call_describe({"quad": 0, "seg_m": 3}, 5) is None
    assert _route({"small_msm": 0, "glv": 1}, 2049) == ("regime A", 8, True)
