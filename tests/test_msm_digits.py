"""The integer model of the MSM front end (tests/msm_digit_model.py) against the product's own exports, without a GPU: its plans
against cg1_plan_describe, its split against cg1_glv_split, and the directed families against what they are built to reach -- every
digit in range, the value reconstructed, no carry out of the top window, and the required events (tie digit, most negative digit, full
carry chain, carry-only top digit) present for every plan.  counts() is checked against a second, naive computation.
Whole file: 25 s on one core (the 26 families of the split, 3 s each at width 4, are most of it)."""
import ctypes
import random

import pytest

import msm_digit_model as M
from curdleproofs_pie_amd import _native as N

R, LAM = M.R, M.LAM


@pytest.mark.parametrize("glv", [0, 1])
def test_model_plan_is_the_engines_plan(glv):
    for c in M.WIDTHS:
        offs = (ctypes.c_int * 80)()
        wid = (ctypes.c_int * 80)()
        nw = N.cg1_plan_describe(c, glv, offs, wid, 80)
        assert nw > 0 and [(offs[w], wid[w]) for w in range(nw)] == M.plan(c, bool(glv)), (c, glv)


def test_model_split_is_the_engines_split():
    for c in (8, 16, -13):
        for k in M.edge_scalars_glv(c):
            assert M.split(k) == M.split_native(k), hex(k)
    for c in (4, 16):                                      # and on the 255-bit family: r - 1, r, r + 1, (r + 1) / 2, 2^255 - 1 are in it
        for k in M.edge_scalars(c):
            assert M.split(k) == M.split_native(k), hex(k)


@pytest.mark.parametrize("c", M.WIDTHS)
def test_family_reconstructs_and_reaches_every_event(c):
    pl = M.plan(c)
    fam = M.edge_scalars(c)                                # (fails by itself if a required event is missing)
    assert 200 <= len(fam) <= 1000 and len(set(fam)) == len(fam)
    for s in fam:
        digits, carry = M.recode(s, pl, 0, with_carry=True)
        assert carry == 0, (c, hex(s))
        assert sum(d << off for d, (off, _) in zip(digits, pl)) == s, (c, hex(s))
        assert all(-(1 << (w - 1)) < d <= 1 << (w - 1) for d, (_, w) in zip(digits, pl)), (c, hex(s))
    ev = M.family_events(fam, pl)
    top = len(pl) - 1
    for w in range(len(pl)):
        assert (("tie", 0, w) in ev) == M.can_hold_tie(pl, w, (1 << 255) - 1), (c, w)      # also: never where it cannot be
        assert w == top or ("most negative", 0, w) in ev, (c, w)
    assert ("carry chain", 0, top) in ev, c
    assert (pl[top][0] == 255) == (c in (5, 15)) and ("carry-only top", 0, top) in ev, c      # (5, 15: a top window with no bit of any scalar)
    # which top windows cannot hold the tie: exactly those of the uniform plans 5 .. 7 and 9 .. 15
    assert M.can_hold_tie(pl, top, (1 << 255) - 1) == (c < 0 or c in (4, 8, 16)), c


@pytest.mark.parametrize("c", M.WIDTHS)
def test_split_family_reconstructs_and_reaches_every_event(c):
    pl = M.plan(c, True)
    fam = M.edge_scalars_glv(c)                            # (asserts split(b lambda + a) == (a, b) and the events of both flips)
    assert len(set(fam)) == len(fam) and all(0 <= s < R for s in fam)
    halves = []
    for s in fam:
        k1, k2 = M.split(s)
        assert (k1 + k2 * LAM - s) % R == 0, hex(s)
        for v in (k1, k2):
            digits, carry = M.recode(abs(v), pl, 1 if v < 0 else 0, with_carry=True)
            assert carry == 0 and M.value_of(digits, pl) == v, (c, hex(s))
            assert all(-(1 << (w - 1)) < d <= 1 << (w - 1) for d, (_, w) in zip(digits, pl)), (c, hex(s))
        halves += [k1, k2]
    ev = M.family_events(halves, pl)
    for flip in (0, 1):
        for w in range(len(pl) - 1):
            assert ("tie", flip, w) in ev and ("most negative", flip, w) in ev, (c, flip, w)
        assert ("carry chain", flip, len(pl) - 1) in ev, (c, flip)
    for row in (0, 1):                                     # both rows run with both flips
        assert {M.split(s)[row] < 0 for s in fam if M.split(s)[row]} == {False, True}


def test_a_broken_recoder_is_not_the_model():
    """The mistakes the families exist to catch, made in a copy of the recoder: each changes a digit of some family scalar."""
    def broken(value, pl, flip, ge=False, no_flip=False):
        digits, carry = [], 0
        for off, w in pl:
            d = ((value >> off) & ((1 << w) - 1)) + carry
            lim = (1 << (w - 1)) - (0 if no_flip else flip)
            if d >= lim if ge else d > lim:
                d, carry = d - (1 << w), 1
            else:
                carry = 0
            digits.append(-d if flip else d)
        return digits
    for c in (16, -13):
        pl = M.plan(c)
        assert any(broken(s, pl, 0, ge=True) != M.recode(s, pl) for s in M.edge_scalars(c))
        plg = M.plan(c, True)
        halves = [v for s in M.edge_scalars_glv(c) for v in M.split(s)]
        assert any(v < 0 and broken(-v, plg, 1, no_flip=True) != M.digits_of(v, plg) for v in halves)


@pytest.mark.parametrize("c,glv,rank,world,L0", [(16, False, 0, 1, 8), (-13, False, 0, 1, 1), (8, True, 0, 1, 2), (9, False, 1, 3, 1)])
def test_counts_against_a_naive_count(c, glv, rank, world, L0):
    rng = random.Random(c * 100 + world)
    pl = M.plan(c, glv)
    few = [rng.randrange(R) for _ in range(3)]             # repeats: loaded buckets, some beyond one chunk
    scalars = [rng.choice(few) if i % 2 else rng.randrange(R) for i in range(400)] + [0, 1, R - 1]
    ident = [i % 7 == 3 for i in range(len(scalars))]
    offsets = [0, 100, 100, 250, len(scalars)] if c == 8 else None
    # the naive count: every (row, window) pair in turn, from the definition of the digits
    entries, per_bucket = 0, {}
    for i, s in enumerate(scalars):
        if ident[i]:
            continue
        g = 0 if offsets is None else max(j for j in range(len(offsets) - 1) if offsets[j] <= i)
        for v in (M.split(s) if glv else (s,)):
            digits = M.digits_of(v, pl)
            assert M.value_of(digits, pl) == v
            for w in range(len(pl)):
                if w % world == rank and digits[w] != 0:
                    entries += 1
                    per_bucket.setdefault((g, w, abs(digits[w])), []).append(i)
    chunks = 0
    for members in per_bucket.values():
        L = L0
        while -(-len(members) // L) > 4096:
            L += 1
        chunks += len([members[k: k + L] for k in range(0, len(members), L)])
    assert M.counts(scalars, ident, pl, glv, rank, world, L0, offsets) == (entries, chunks)
    assert entries >= chunks > 0 and (entries > chunks) == (L0 > 1)      # (chunks of one entry: no mixed addition at all)


def test_chunk_count_edges():
    for L0 in (1, 8):
        # 4096 L0 + 1 entries: the chunks grow to L0 + 1 entries, 2 049 chunks of 2 or 3 641 of 9
        want = {1: 1, L0: 1, L0 + 1: 2, 2 * L0: 2, 16 * L0: 16, 16 * L0 + 1: 17, 17 * L0: 17, 4096 * L0: 4096, 4096 * L0 + 1: {1: 2049, 8: 3641}[L0]}
        for cnt, nch in want.items():
            assert M.chunk_count(cnt, L0) == nch, (L0, cnt)
    assert M.chunk_count(0, 8) == 0 and M.chunk_count(7, 8) == 1
    assert M.call_chunk_len(8, 32769, 16) == 8 and M.call_chunk_len(1, 4097, 32) == 1
    assert M.call_chunk_len(8, 32768, 32) == 10 and M.call_chunk_len(8, 32768, 32, chunk_rule=False) == 8
    assert M.call_chunk_len(1, 1 << 15, 32, chunk_rule=False) == 4 and M.call_chunk_len(1, 1 << 15, 32, world=2) == 4      # 2^20 rows x windows = 4 x 2^18


def _described_chunk_len(L0, rows, c, world=1, chunk_rule=1):
    d = N.msm_call_describe({"small_msm": 0, "chunk_len": L0, "chunk_rule": chunk_rule}, rows, c, 0, world)
    assert d["engine"] == "regime A" and d["c"] == c and not d["glv"]
    return d["chunk_len"]


@pytest.mark.parametrize("L0", [1, 8, 64])
@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("chunk_rule", [0, 1])
def test_call_chunk_len_is_the_planners(L0, world, chunk_rule):
    """The planner's chunk length (cg1_msm_call_describe) == the model's, one row below, at and one row above every point where rows x
    windows crosses 2^18 L0 (the first doubling), 2^20 and 2^21 (the rules' edges), whole plan and rank 0 of 2 of the 16 windows of c = 16."""
    nlw = 16 // world
    for edge in ((1 << 18) * L0, 1 << 20, 1 << 21):
        for rows in (edge // nlw - 1, edge // nlw, edge // nlw + 1):
            want = M.call_chunk_len(L0, rows, nlw, world, bool(chunk_rule), cmax=16)
            assert _described_chunk_len(L0, rows, 16, world, chunk_rule) == want, (L0, world, chunk_rule, rows, want)


def test_whole_bucket_chunks_under_the_automatic_plan():
    """The third rule -- a chunk holds a whole bucket between 2^21 and 2^24 rows x windows -- at 2^17, 2^18 and 2^19 rows under the plan
    window_c = 0 picks (-15, 16, 16), on both sides of 2^22 rows x windows, where the cap of 20 ends, and of its two outer edges.  The
    lengths are written out: mean load 8 -> 8 + 8 sqrt 8 + 1 = 31 (capped: 20), mean load 16 -> 49."""
    for rows, c, nwin, want in ((1 << 17, -15, 18, 20), (1 << 18, 16, 16, 31), (1 << 19, 16, 16, 49)):
        d = N.msm_call_describe({}, rows, 0)
        assert (d["engine"], d["c"], d["chunk_len"]) == ("regime A", c, want), (rows, d)
        assert M.call_chunk_len(8, rows, nwin, cmax=abs(c)) == want, rows
    assert M.call_chunk_len(8, (1 << 18) - 1, 16, cmax=16) == 20 and M.call_chunk_len(8, 1 << 18, 16, cmax=16) == 31      # 2^22 rows x windows
    for rows in ((1 << 17) - 1, 1 << 17, (1 << 18) - 1, 1 << 18, (1 << 20) - 1, 1 << 20):       # 2^21, 2^22 and 2^24 rows x windows at c = 16
        for L0 in (1, 8, 64):
            assert _described_chunk_len(L0, rows, 16) == M.call_chunk_len(L0, rows, 16, cmax=16), (rows, L0)
    # sharded, switched off, or with the quad tail taking every bucket ("rowcol_quad_max"): the first rule alone
    assert M.call_chunk_len(8, 1 << 18, 8, world=2, cmax=16) == M.call_chunk_len(8, 1 << 18, 16, chunk_rule=False, cmax=16) - 8 == 8
    assert M.call_chunk_len(8, 1 << 18, 16, cmax=16, rowcol_quad_max=1 << 19) == 16
    assert N.msm_call_describe({"rowcol_quad_max": 1 << 19}, 1 << 18, 16)["chunk_len"] == 16


@pytest.mark.parametrize("c", [8, 16, -13])
def test_bucket_load_cases_load_what_they_say(c):
    pl = M.plan(c)
    for L0 in (1, 8):
        cases = M.bucket_load_cases(c, L0)
        seen = set()
        for label, sc in cases:
            cnt = int(label.split()[1].rstrip(","))
            buckets = {}
            for s in set(sc):
                (w, d), = [(w, d) for w, d in enumerate(M.recode(s, pl)) if d]
                assert d > 0
                buckets[(w, d)] = sc.count(s)
            assert set(buckets.values()) == {cnt}, label
            seen |= {(cnt, w, d) for w, d in buckets}
            assert M.counts(sc, [False] * len(sc), pl, L0=L0) == (cnt * len(buckets), M.chunk_count(cnt, L0) * len(buckets))
        for cnt in M.bucket_loads(L0):
            if cnt:
                assert (cnt, 0, 1 << (abs(c) - 1)) in seen, (c, L0, cnt)      # the tie bucket of window 0
                assert any(k[0] == cnt and k[1] == len(pl) - 1 for k in seen), (c, L0, cnt)
        sc = M.mixed_load_case(c, L0)
        assert M.counts(sc, [False] * len(sc), pl, L0=L0) == (3 * (51 * L0 + 1), 3 * (2 + 17 + 16 + 17))
        world = {8: 3, 16: 2, -13: 2}[c] if L0 == 1 else 1
        sc, own = M.heavy_list_case(c, L0, world)
        e, ch = M.counts(sc, [False] * len(sc), pl, rank=0, world=world, L0=L0)
        assert e == len(sc) * len(own) and ch == 17 * (e // (16 * L0 + 1)) and e // (16 * L0 + 1) == len(sc) * len(own) // (16 * L0)
