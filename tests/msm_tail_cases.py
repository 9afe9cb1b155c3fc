"""The reduction tail of the MSM engine -- everything between k_accumulate and the final point -- restated for the tests: which kernels a
call launches (tail_path and its counterparts for regime B and k_msm_small: csrc/host_chains.h's decisions in plain Python, returning the
dict Context.last_tail() returns), the input families that make every correct tail, however it is shaped, add a point to itself and to
its negative, and the list of switch settings that reaches every leaf of every choice.  No GPU and no product code here; shared by
tests/test_msm_tail.py (host) and tests/test_msm_tail_gpu.py (device).

A term is (scalar, k): the scalar under the base k G.  A term m 2^off_w with m <= 2^(width - 1) has exactly one non-zero digit, m, in
window w (msm_digit_model.bucket_load_cases' construction), so it lands in bucket b = m - 1 of that window and nowhere else; a "negative"
entry is the base (r - k) G under the same positive digit.  The expected point of a case is (sum k_i s_i mod r) G; nothing here has a
tolerance.  Bucket b lies in row b >> lb and column b & (2^lb - 1), lb = ceil((cmax - 1) / 2) (k_rowcol); the tail exports per window
T0 = sum of all buckets (weight 2^off), one masked sum per column bit k (2^(off + k)) and per row bit k (2^(off + lb + k)).

What a family guarantees is ASSERTED from the digit model when it is built (check_family), not hoped for."""
import functools

import msm_digit_model as M
from oracle import bls12_381 as O

R = M.R
K = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % R          # P = K G
TOP = (1 << 255) - 1
HEAVY = M.HEAVY_MIN_CHUNKS

DEFAULT_PARAMS = {"reduce_2d": 1, "quad": 1, "rowcol_quad": 1, "rowcol_quad_max": 1 << 18, "rowcol_row": 1, "tree_row": 1, "fold_quad": 1, "fold_pass": 1,
                  "rowcol_lgq": 0, "tree_shift": 2, "tree_half": 1, "zero_copy": 1, "seg_m": 4, "host_split": 1, "horner_threads": 4,
                  "horner_row": 1, "batched_host_horner_max": 24, "small_row_tail": 1}
ROWS_FOLD_MAX = 8192                # k_rowcol_quad_row adds a bucket's chunk sums itself up to this many buckets
HORNER_ROW_MAX = 2048               # regime B: one wave per MSM up to this many MSMs


# ------------------------------------------------------------------ which tail runs
def geometry(c):
    """(bucket bits, lb, hb) of a plan: the 2-D split of the bucket index is the widest window's."""
    bb = abs(c) - 1
    lb = (bb + 1) // 2
    return bb, lb, bb - lb


def _tail(**kw):
    d = {"fold": None, "rowcol": None, "lgq": 0, "rowcol_use_quad": 0, "seg_m": 0, "tree": None, "tree_waves": 0, "export": None, "horner": None,
         "horner_threads": 0, "small_row_tail": None}
    d.update(kw)
    return d


def host_threads(p, e_top):
    """Threads of regime A's host Horner: one below bit 96 or without "host_split", four from bit 112 on when "horner_threads" allows."""
    if not p["host_split"] or e_top < 96:
        return 1
    return 4 if p["horner_threads"] >= 4 and e_top >= 112 else 2


def tail_path(c, nlw, n, params, e_top=0):
    """What msm_enqueue / msm_finish launch behind k_accumulate for a regime-A call of n terms that owns nlw windows of plan c, under
    `params` (over DEFAULT_PARAMS), when the highest exported point that is not the identity has weight 2^e_top.  n takes no part: the
    tail is chosen from the bucket count alone."""
    p = dict(DEFAULT_PARAMS, **params)
    bb, lb, hb = geometry(c)
    nb_total = nlw << bb
    use2d = bool(p["reduce_2d"])
    small_quad = bool(p["quad"] and p["rowcol_quad"] and nb_total <= p["rowcol_quad_max"])
    row_pair = bool(p["rowcol_row"] and p["tree_row"])
    rows_fold = small_quad and use2d and row_pair and nb_total <= ROWS_FOLD_MAX
    # k_rowcol_quad reads only the first slot of a bucket: a fold runs in front of it whatever "fold_pass" says
    if rows_fold:
        fold = None
    elif small_quad and p["fold_quad"]:
        fold = "k_bucket_fold_quad"
    elif p["fold_pass"] or (small_quad and use2d and not row_pair):
        fold = "k_bucket_fold"
    else:
        fold = None
    t = _tail(fold=fold, horner="host", horner_threads=host_threads(p, e_top))
    if not use2d:
        t.update(rowcol="k_seg_reduce", seg_m=min(p["seg_m"], 1 << bb), export="k_export_host" if p["zero_copy"] else "hipMemcpyAsync")
        return t
    if small_quad and row_pair:
        t["rowcol"] = "k_rowcol_quad_row"
    elif small_quad:
        t.update(rowcol="k_rowcol_quad", lgq=p["rowcol_lgq"] if 2 <= p["rowcol_lgq"] <= 4 else (2 if hb == lb else 3))
    else:
        t.update(rowcol="k_rowcol", rowcol_use_quad=1 if p["quad"] else 0)
    if p["tree_row"]:
        t.update(tree="k_small_tree_row", tree_waves=min(16, max(1, (1 << max(hb, lb)) >> 3)))
    elif p["quad"]:
        shift = p["tree_shift"] if p["tree_shift"] >= 0 else (1 if p["tree_half"] else 0)
        t.update(tree="k_small_tree_quad", tree_waves=max(64, min(512, max(64, 4 << max(hb, lb)) >> shift)) >> 6)
    else:
        t.update(tree="k_small_tree", tree_waves=4)
    t["export"] = ("k_small_tree_row" if p["tree_row"] else "k_export_host") if p["zero_copy"] else "hipMemcpyAsync"
    return t


def tail_path_batched(c, M_, params):
    """Regime B (batched_chain_enqueue) over M_ MSMs at width c: k_seg_reduce + k_group_reduce, then the Horner of every MSM."""
    p = dict(DEFAULT_PARAMS, **params)
    t = _tail(rowcol="k_seg_reduce", seg_m=min(8, 1 << (c - 1)), export="hipMemcpyAsync")
    if M_ <= p["batched_host_horner_max"]:
        t.update(horner="host", horner_threads=min(4, M_))
    elif p["horner_row"] and M_ <= HORNER_ROW_MAX:
        t["horner"] = "k_msm_horner_row"
    else:
        t["horner"] = "k_msm_horner_quad" if p["quad"] else "k_msm_horner"
    return t


def tail_path_small(M_, params, e_top=0):
    """k_msm_small: its own tail behind "small_row_tail"; the Horner on the host -- msm_finish's for one MSM, one thread per MSM for up to
    four, the worker pool (reported as 0 threads) beyond."""
    p = dict(DEFAULT_PARAMS, **params)
    nth = host_threads(p, e_top) if M_ == 1 else (M_ if M_ <= 4 else 0)
    return _tail(small_row_tail=1 if p["small_row_tail"] else 0, horner="host", horner_threads=nth)


# ------------------------------------------------------------------ what a list of terms puts where
def all_buckets(terms, pl):
    """[{bucket: (log of its sum mod r, entries)} per window], from the digit model (not from how the terms were built)."""
    out = [{} for _ in pl]
    for s, k in terms:
        for w, d in enumerate(M.recode(s, pl)):
            if d:
                lg, cnt = out[w].get(abs(d) - 1, (0, 0))
                out[w][abs(d) - 1] = ((lg + (k if d > 0 else -k)) % R, cnt + 1)
    return out


def row_col_logs(bk, c):
    """-> ({row: log}, {column: log}) of a window's buckets: every row / column that holds an entry, its sum's log mod r."""
    _, lb, _ = geometry(c)
    rows, cols = {}, {}
    for b, (lg, _) in bk.items():
        rows[b >> lb] = (rows.get(b >> lb, 0) + lg) % R
        cols[b & ((1 << lb) - 1)] = (cols.get(b & ((1 << lb) - 1), 0) + lg) % R
    return rows, cols


def item_logs(bk, c, off, reduce_2d=1, seg_m=4):
    """[(exponent, log)] of the points the tail exports for one window at bit offset `off`: the 2-D items, or the 1-D fallback's
    (T = sum of the segments' running sums, one masked sum of segment totals per segment-index bit)."""
    bb, lb, hb = geometry(c)
    masked = lambda d, k: sum(v for i, v in d.items() if (i >> k) & 1) % R
    if reduce_2d:
        rows, cols = row_col_logs(bk, c)
        return [(off, sum(rows.values()) % R)] + [(off + lb + k, masked(rows, k)) for k in range(hb)] + [(off + k, masked(cols, k)) for k in range(lb)]
    m = min(seg_m, 1 << bb)
    lm = m.bit_length() - 1
    tot = {}
    for b, (lg, _) in bk.items():
        tot[b // m] = (tot.get(b // m, 0) + lg) % R
    tot = {j: v for j, v in tot.items() if v}
    return [(off, sum((b % m + 1) * lg for b, (lg, _) in bk.items()) % R)] + [(off + lm + k, masked(tot, k)) for k in range(bb - lm)]


class Case:
    """One input: its family, a label for messages, the terms, the window the family sits in (None: several), and what the digit model
    makes of it -- the buckets of every window, the log of the point (whole plan or a shard), the top exponent of the exported points."""

    def __init__(self, c, family, label, terms, w):
        self.c, self.family, self.label, self.terms, self.w = c, family, label, terms, w
        self.pl = M.plan(c)
        self.buckets = all_buckets(terms, self.pl)
        self._top = {}

    def log(self, windows=None):
        """log of the case's point over `windows` (None: all): sum over the buckets of digit x bucket sum x 2^offset; over the whole
        plan that is sum k s, asserted."""
        ws = range(len(self.pl)) if windows is None else windows
        v = sum(((b + 1) * lg) << self.pl[w][0] for w in ws for b, (lg, _) in self.buckets[w].items()) % R
        if windows is None:
            assert v == sum(k * s for s, k in self.terms) % R, self.label
        return v

    def e_top(self, params, windows=None):
        """The highest exponent of an exported point that is not the identity (what msm_finish sizes its thread count from), 0 if none.
        The exported points' weighted sum is the case's own point: asserted."""
        p = dict(DEFAULT_PARAMS, **params)
        key = (p["reduce_2d"], 0 if p["reduce_2d"] else p["seg_m"], None if windows is None else tuple(windows))
        if key not in self._top:
            top, total = 0, 0
            for w in (range(len(self.pl)) if windows is None else windows):
                for e, lg in item_logs(self.buckets[w], self.c, self.pl[w][0], p["reduce_2d"], p["seg_m"]):
                    total += lg << e
                    if lg:
                        top = max(top, e)
            assert total % R == self.log(windows), self.label
            self._top[key] = top
        return self._top[key]


def expected_point(log):
    return O.g1_compress(O.g1_mul(O.G1_GEN, log) if log else None)


# ------------------------------------------------------------------ the families
def avail(pl, w):
    """Buckets of window w a one-digit term can reach: 2^(width - 1), fewer where the window runs into bit 255."""
    off, wd = pl[w]
    return min(1 << (wd - 1), TOP >> off)


def term(pl, w, b, k):
    off, _ = pl[w]
    s = (b + 1) << off
    assert 0 <= b < avail(pl, w) and 0 < s <= TOP
    return (s, k % R)


def top_window(c):
    """The highest window a one-digit term can reach two buckets of (width 5's last window holds nothing but the recoding carry)."""
    pl = M.plan(c)
    return max(w for w in range(len(pl)) if avail(pl, w) >= 2)


def placements(c):
    """The windows a family is placed in: the first, a middle one and the top one."""
    return tuple(dict.fromkeys((0, len(M.plan(c)) // 2, top_window(c))))


def fam_equal(c, w):
    """Every bucket of window w holds P once: all row sums are equal and all column sums are equal (where the window's bucket count is
    a whole number of rows), so every pairwise level of a tree adds a point to itself."""
    pl = M.plan(c)
    return [term(pl, w, b, K) for b in range(avail(pl, w))]


def fam_alternating(c, w):
    """P in even buckets, -P in odd ones: every whole row sums to the identity, column sums alternate +-, and of the bit-masked items only
    bit 0 of the column index survives."""
    pl = M.plan(c)
    return [term(pl, w, b, K if b % 2 == 0 else -K) for b in range(avail(pl, w))]


def fam_mirror(c, w):
    """Column l holds the negation of column Cn - 1 - l, and (where the whole rows are even in number) row h that of row Rw - 1 - h, at three
    magnitudes: the pairs sit far apart, so the sums cancel in the cross-lane levels of a tree, not in a lane's serial part.  One more P
    in bucket 0 keeps the case's point off the identity."""
    pl = M.plan(c)
    _, lb, _ = geometry(c)
    Cn = 1 << lb
    Rw = avail(pl, w) // Cn
    out = []
    for h in range(Rw):
        for l in range(Cn):
            sgn = (1 if l < Cn // 2 else -1) * ((1 if h < Rw // 2 else -1) if Rw % 2 == 0 else 1)
            mag = 1 + (min(h, Rw - 1 - h) * Cn + min(l, Cn - 1 - l)) % 3
            out.append(term(pl, w, h * Cn + l, sgn * mag * K))
    return out + [term(pl, w, 0, K)]


def fam_sparse(c, w):
    """{name: terms}: one case each -- only bucket 0 (in no masked item), only bucket 1, only the last bucket (the tie digit where the
    window can hold it), one full row alone, one full column alone, the last row plus the last column."""
    pl = M.plan(c)
    _, lb, _ = geometry(c)
    Cn = 1 << lb
    na = avail(pl, w)
    Rw = max(1, na // Cn)
    row = lambda h: [term(pl, w, h * Cn + l, K) for l in range(Cn) if h * Cn + l < na]
    col = lambda l: [term(pl, w, h * Cn + l, K) for h in range(Rw) if h * Cn + l < na]
    out = {"bucket 0": [term(pl, w, 0, K)], "bucket 1": [term(pl, w, 1, K)], "last bucket": [term(pl, w, na - 1, K)],
           "one row": row(Rw - 1), "one column": col(Cn - 2), "last row + last column": row(Rw - 1) + col(Cn - 1)[: Rw - 1]}
    return {k: v for k, v in out.items() if v}                 # (a top window of a few buckets has no column Cn - 2)


def fam_windows(c):
    """{name: terms} over several windows: an empty window between two full ones, everything empty but the top window."""
    pl = M.plan(c)
    mid = len(pl) // 2
    return {"empty window between two full ones": fam_equal(c, mid - 1) + fam_equal(c, mid + 1),
            "only the top window": fam_equal(c, top_window(c))}


CHUNK_LOADS = (2, 3, 16, 17, 18)


def fam_chunks(c, w):
    """Buckets 0 .. 4 of window w hold j = 2, 3, 16, 17, 18 copies of P: at chunk lengths 1 and 2 their chunk sums are equal (the fold and
    the heavy combine double); buckets 5 .. 9 hold P, -P, P, -P, ... of the same lengths: at chunk length 2 identity chunk sums among
    finite ones, at 1 opposite neighbours."""
    pl = M.plan(c)
    assert avail(pl, w) >= 10 or c == 4
    out = []
    for i, j in enumerate(CHUNK_LOADS):
        if i < avail(pl, w):
            out += [term(pl, w, i, K)] * j
        if 5 + i < avail(pl, w):
            out += [term(pl, w, 5 + i, K if t % 2 == 0 else -K) for t in range(j)]
    return out


def fam_horner(c):
    """{name: terms}: one entry (bucket 0) per window, so that a window's sum is its only exported point.  "doubling": from a start window
    down, every window's sum equals the accumulator after its doublings -- W_w = 2^width_w acc_(w+1) -- so each addition of the Horner is
    a doubling; "cancel": W_w = -2^width_w acc_(w+1), the accumulator becomes the identity and the window below revives it; "vanish": the same without the
    reviving window -- the call's point is the identity; "empty top":
    nothing above the middle; "empty lowest": nothing in window 0."""
    pl = M.plan(c)
    n = top_window(c) + 1
    hi = min(n - 1, n // 2 + 2)
    dbl, acc = [], 0
    for w in range(hi, hi - 4, -1):
        k = K if w == hi else (acc << pl[w][1]) % R
        dbl.append(term(pl, w, 0, k))
        acc = ((acc << pl[w][1]) + k) % R
    cancel = [term(pl, hi, 0, K), term(pl, hi - 1, 0, -(K << pl[hi - 1][1])), term(pl, hi - 2, 0, 3 * K)]
    return {"doubling": dbl, "cancel": cancel, "vanish": cancel[:2],
            "empty top": [term(pl, w, 0, (w + 1) * K) for w in range(0, n // 2)],
            "empty lowest": [term(pl, w, 0, (w + 2) * K) for w in range(1, n, max(1, n // 6))]}


def check_family(case, L0=8):
    """The property that makes the case's family meet its exceptional additions in ANY correct tail, asserted from the digit model; only
    its window may hold anything (the multi-window families: one entry per window, or whole windows).  -> the buckets of its window."""
    name, c, w, pl = case.family, case.c, case.w, case.pl
    _, lb, _ = geometry(c)
    Cn = 1 << lb
    bk = case.buckets[w] if w is not None else {}
    if w is not None:
        assert all(not case.buckets[v] for v in range(len(pl)) if v != w), (name, c, w)
        rows, cols = row_col_logs(bk, c)
        whole = avail(pl, w) % Cn == 0
    if name == "equal":
        assert len(bk) == avail(pl, w) and {v for v in bk.values()} == {(K, 1)}, (c, w)
        if whole:
            assert len(set(rows.values())) == 1 and len(set(cols.values())) == 1, (c, w)
    elif name == "alternating":
        assert len(bk) == avail(pl, w)
        if whole:
            assert set(rows.values()) == {0}, (c, w)
        assert all((v == 0) or (v in ((len(rows) * K) % R, -(len(rows) * K) % R, ((len(rows) - 1) * K) % R, -((len(rows) - 1) * K) % R)) for v in cols.values())
        live = [(e, lg) for e, lg in item_logs(bk, c, pl[w][0]) if lg]
        if whole:
            assert [e for e, _ in live] == [pl[w][0]], (c, w, live)        # only bit 0 of the column index survives
    elif name == "mirror":
        r0 = rows.pop(0)
        c0 = cols.pop(0)
        assert set(rows.values()) <= {0} and r0 == K, (c, w)
        if (avail(pl, w) // Cn) % 2 == 0:                                  # mirrored across the rows as well
            assert set(cols.values()) <= {0} and c0 == K, (c, w)
        assert len({lg for lg, _ in bk.values()}) >= 3                     # both signs of several magnitudes
    elif name == "sparse":
        kind = case.label.split(": ")[1].split(",")[0]
        want = {"bucket 0": (1, 1), "bucket 1": (1, 1), "last bucket": (1, 1), "one row": (1, None), "one column": (None, 1)}.get(kind)
        if want:
            assert (want[0] is None or len(rows) == want[0]) and (want[1] is None or len(cols) == want[1]) and set(v for v, _ in bk.values()) == {K}, case.label
        else:                                                              # last row + last column: they share no bucket twice
            assert all(v == (K, 1) for v in bk.values()) and (not whole or len(bk) == Cn + len(rows) - 1), case.label
    elif name == "horner":
        assert all(len(b) <= 1 and all(k == 0 for k in b) for b in case.buckets), case.label      # a window's sum is its only exported point
        if case.label.endswith("doubling") or case.label.endswith("cancel"):
            acc, seen = 0, []
            for wv in range(len(pl) - 1, -1, -1):
                acc = (acc << pl[wv][1]) % R
                if case.buckets[wv]:
                    seen.append("double" if acc and case.buckets[wv][0][0] == acc else ("cancel" if acc and (case.buckets[wv][0][0] + acc) % R == 0 else "add"))
                    acc = (acc + case.buckets[wv][0][0]) % R
            assert seen == (["add", "double", "double", "double"] if case.label.endswith("doubling") else ["add", "cancel", "add"]), (case.label, seen)
    elif name == "windows":
        filled = [wv for wv in range(len(pl)) if case.buckets[wv]]
        assert filled in ([len(pl) // 2 - 1, len(pl) // 2 + 1], [top_window(c)]), (case.label, filled)
    elif name == "chunks":
        got = sorted(cnt for _, cnt in bk.values())
        assert set(got) <= set(CHUNK_LOADS) and got.count(17) >= 1, (c, w, got)
        nch = sorted(M.chunk_count(cnt, L0) for _, cnt in bk.values())
        assert max(nch) >= HEAVY - (L0 > 1) * HEAVY // 2 and 2 in nch, (c, w, L0, nch)
        if L0 == 1:
            assert HEAVY in nch and HEAVY - 1 in nch and HEAVY + 1 in nch       # both sides of the fold / heavy-combine threshold
    return bk


# ------------------------------------------------------------------ the cases of a width
def max_filled_windows(c):
    """Full families need 2^(cmax - 1) terms per filled window: three windows up to width 10, one from 11 on (32 768 terms at most)."""
    return 3 if abs(c) <= 10 else 1


@functools.lru_cache(maxsize=None)
def cases(c, full=True):
    """The Cases of plan c.  full: the three dense families in every placement; else only in the middle
    window (the switch products run the short list)."""
    pl = M.plan(c)
    n = len(pl)
    mid = n // 2
    out = []
    where = placements(c) if full and max_filled_windows(c) >= 3 else (mid,)
    for w in where:
        for name, fam in (("equal", fam_equal), ("alternating", fam_alternating), ("mirror", fam_mirror)):
            if name != "mirror" or avail(pl, w) >= 1 << geometry(c)[1]:          # (a whole row at least)
                out.append((name, f"{name}, window {w}", fam(c, w), w))
    if full and max_filled_windows(c) < 3:                 # the other placements: the alternating family alone
        out += [("alternating", f"alternating, window {w}", fam_alternating(c, w), w) for w in placements(c) if w != mid]
    for name, t in fam_sparse(c, mid).items():
        out.append(("sparse", f"sparse: {name}, window {mid}", t, mid))
    if full:
        for name, t in fam_sparse(c, top_window(c)).items():
            out.append(("sparse", f"sparse: {name}, window {top_window(c)}", t, top_window(c)))
        if max_filled_windows(c) >= 3:
            for name, t in fam_windows(c).items():
                out.append(("windows", f"windows: {name}", t, None))
    for name, t in fam_horner(c).items():
        out.append(("horner", f"horner: {name}", t, None))
    out = [Case(c, name, label, t, w) for name, label, t, w in out]
    for case in out:
        check_family(case)
    return out


def chunk_cases(c):
    """The chunks family in the first, a middle and the top window, where the window has ten buckets."""
    pl = M.plan(c)
    return [Case(c, "chunks", f"chunks, window {w}", fam_chunks(c, w), w) for w in placements(c) if avail(pl, w) >= 10]


# ------------------------------------------------------------------ the switch settings
FOLDS = ({"fold_quad": 1, "fold_pass": 1}, {"fold_quad": 0, "fold_pass": 1}, {"fold_quad": 0, "fold_pass": 0}, {"fold_quad": 1, "fold_pass": 0})
SUSPECT = {"fold_quad": 0, "fold_pass": 0, "rowcol_row": 0}        # no fold in front of k_rowcol_quad before the fix in msm_enqueue
TRIPLE_WIDTHS = (4, 8, 9, 14)


def triples():
    """Every legal (fold, row / column, tree) combination as switch settings: the four fold settings under k_rowcol_quad_row, k_rowcol_quad at
    every lgq with both trees that can read its sums, k_rowcol with and without quads under the trees each allows, and the 1-D form."""
    out = []
    for f in FOLDS:
        out.append(dict(f))                                                                    # k_rowcol_quad_row + k_small_tree_row
        for lgq in (2, 3, 4):
            out.append(dict(f, rowcol_lgq=lgq, rowcol_row=0))                                  # k_rowcol_quad + k_small_tree_row
            out.append(dict(f, rowcol_lgq=lgq, tree_row=0))                                    # k_rowcol_quad + k_small_tree_quad
        out.append(dict(f, rowcol_quad=0))                                                     # k_rowcol (quads) + k_small_tree_row
        out.append(dict(f, rowcol_quad=0, tree_row=0))                                         # k_rowcol (quads) + k_small_tree_quad
        out.append(dict(f, quad=0))                                                            # k_rowcol (lanes) + k_small_tree_row
        out.append(dict(f, quad=0, tree_row=0))                                                # k_rowcol (lanes) + k_small_tree
        out.append(dict(f, reduce_2d=0))                                                       # k_seg_reduce + the bit trees
    return out


def leaves():
    """A short list that launches every leaf of the four choices at least once: run at every width."""
    out = [{}, dict(SUSPECT), {"tree_row": 0}, {"tree_row": 0, "fold_quad": 0}, {"rowcol_quad": 0}, {"rowcol_quad": 0, "fold_pass": 0}, {"quad": 0},
           {"quad": 0, "tree_row": 0}, {"quad": 0, "tree_row": 0, "zero_copy": 0}, {"reduce_2d": 0}, {"reduce_2d": 0, "fold_quad": 0, "fold_pass": 0},
           {"zero_copy": 0}, {"tree_row": 0, "zero_copy": 0}, {"reduce_2d": 0, "zero_copy": 0}]
    out += [{"rowcol_row": 0, "rowcol_lgq": q} for q in (2, 3, 4)]
    out += [{"tree_row": 0, "tree_shift": s} for s in (0, 1, 3, 4)] + [{"tree_row": 0, "tree_shift": -1, "tree_half": h} for h in (0, 1)]
    out += [{"reduce_2d": 0, "seg_m": m} for m in (1, 2, 8, 16)]
    return out


def configs(c):
    """[(params, shard)] for plan c, beside the products of triples() at TRIPLE_WIDTHS; shard = None (the whole plan) or a window w run as the one-window shard (w, nwin).  "rowcol_quad_max":
    -1 / -2 stand for the call's bucket count and one less (resolve()).  Plans too large for the default "rowcol_quad_max" (widths 15, 16)
    run the quad leaves with it raised to their bucket count."""
    nwin = len(M.plan(c))
    mid = nwin // 2
    big = (nwin << (abs(c) - 1)) > DEFAULT_PARAMS["rowcol_quad_max"]
    base = [dict(p, rowcol_quad_max=-1) if big and p.get("quad", 1) and p.get("rowcol_quad", 1) else p for p in leaves()]
    out = [(p, None) for p in base]
    if big:
        out.append(({}, None))                                                              # the default of such a plan: k_rowcol
    # both sides of "rowcol_quad_max", in both fold settings that matter there, whole plan and one-window shard
    for shard in (None, mid):
        for f in ({}, {"fold_quad": 0, "fold_pass": 0}):
            out += [(dict(f, rowcol_quad_max=-1), shard), (dict(f, rowcol_quad_max=-2), shard), (dict(f, rowcol_quad_max=-2, tree_row=0), shard)]
    # one-window shards: nb_total = 2^(cmax - 1) exactly; widths 14 and 15 sit on the two sides of the rows' own fold (8192 buckets)
    out += [(p, mid) for p in ({}, {"fold_quad": 0}, {"fold_quad": 0, "fold_pass": 0}, dict(SUSPECT), {"tree_row": 0}, {"reduce_2d": 0})]
    seen, uniq = set(), []
    for p, s in out:
        key = (tuple(sorted(p.items())), s)
        if key not in seen:
            seen.add(key)
            uniq.append((p, s))
    return uniq


def resolve(params, c, nlw):
    """params with the bucket-count stand-ins of "rowcol_quad_max" filled in for a call that owns nlw windows."""
    p = dict(params)
    if p.get("rowcol_quad_max", 0) < 0:
        p["rowcol_quad_max"] = (nlw << (abs(c) - 1)) + 1 + p["rowcol_quad_max"]
    return p


ALL_WIDTHS = tuple(range(4, 17)) + (-13, -16)

# host Horner threads: (plan, top window of a one-entry-per-window case) -> e_top on both sides of 96 and of 112
HORNER_TOPS = ((8, 11), (8, 12), (8, 13), (8, 14), (8, 15), (4, 23), (4, 24), (4, 27), (4, 28), (16, 5), (16, 6), (16, 7), (16, 15))


def horner_thread_case(c, wtop):
    """One entry in bucket 0 of every third window up to wtop: the top exported point is T0 of window wtop, weight 2^offset."""
    pl = M.plan(c)
    return [term(pl, w, 0, (w + 1) * K) for w in range(wtop % 3, wtop + 1, 3)]


HORNER_THREAD_PARAMS = tuple({"horner_threads": t, "host_split": h} for t in (1, 2, 4) for h in (1, 0))

# regime B: M on both sides of the host bound (24) and of the one-wave-per-MSM bound (2048), and the bound moved to M and M - 1
BATCHED_M = (24, 25, 2048, 2049)


def batched_params(M_):
    out = [{"horner_row": hr, "quad": q} for hr in (1, 0) for q in (1, 0)]
    return out + [{"batched_host_horner_max": M_}, {"batched_host_horner_max": M_ - 1}, {"batched_host_horner_max": M_ - 1, "horner_row": 0},
                  {"batched_host_horner_max": M_ - 1, "horner_row": 0, "quad": 0}]


def batched_case(c, M_):
    """M_ MSMs of 2 .. 4 terms from the sparse, equal and Horner families, in turn -> (terms, offsets): a lone bucket, the same base twice in
    one bucket, P and -P in one bucket (an identity window sum), a doubling Horner step, a cancelling one with and without a reviving window (the identity), an MSM whose top windows are empty."""
    pl = M.plan(c)
    n = len(pl)
    w1 = pl[n - 2][1]
    kinds = (                                                  # (j enters through a few residues only: few distinct expected points)
        lambda j: [term(pl, j % n, (j % 5) % avail(pl, j % n), K), term(pl, (j + 1) % n, 0, 2 * K)],
        lambda j: [term(pl, j % 3, 1, K)] * 2 + [term(pl, 0, 0, K)],
        lambda j: [term(pl, j % 4, 2, K), term(pl, j % 4, 2, -K), term(pl, n - 1, 0, (j % 7 + 1) * K)],
        lambda j: [term(pl, n - 1, 0, K), term(pl, n - 2, 0, K << w1)],
        lambda j: [term(pl, n - 1, 0, K), term(pl, n - 2, 0, -(K << w1)), term(pl, j % 5, 0, 5 * K), term(pl, j % 5, 1, K)],
        lambda j: [term(pl, 0, j % avail(pl, 0), K), term(pl, 1, 0, -K)],
        lambda j: [term(pl, n - 1, 0, K), term(pl, n - 2, 0, -(K << w1))],
    )
    terms, offs = [], [0]
    for j in range(M_):
        t = kinds[j % len(kinds)](j % 55)
        assert 2 <= len(t) <= 4
        terms += t
        offs.append(len(terms))
    return terms, offs
