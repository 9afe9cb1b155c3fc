"""tests/msm_tail_cases.py checked on the host: the families have the properties that force doublings and cancellations in any correct
reduction tail, their closed forms are what the oracle's compute_MSM gives, and the configuration list reaches every leaf of every choice
the tail makes, with a call on each side of every threshold.  No GPU."""
import pytest

import msm_digit_model as M
import msm_tail_cases as T
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
