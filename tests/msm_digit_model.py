"""An exact integer model of everything an MSM call does BEFORE k_accumulate -- the window plan (make_plan), the signed-digit recoding
(DigitIter::next), the endomorphism split (glv.h), the window shards, the bucket sort and the chunk plan (call_chunk_len / chunk_count) -- and
the directed scalar families that drive every rare branch of it, shared by tests/test_msm_digits.py (host) and
tests/test_msm_digits_gpu.py (device).  Plain Python on integers, written from the comments of the C++ and not from its code; the only
product code here is split_native(), the ctypes wrapper of cg1_glv_split the tests compare split() with.

What the two counters of cg1_get_last_counts mean, exactly (counts() below):
  entries  the non-zero digits of terms whose base is not the identity, over the windows the call owns; with the split both half-rows
           count and row n + i carries term i's identity flag
  chunks   a bucket is (MSM of a batched call, local window, |digit|); one with cnt entries is cut into ceil(cnt / L) chunks,
           L = max(L0, ceil(cnt / 4096)); chunks is the sum over the non-empty buckets
mixed additions = entries - chunks is what bench.py reports per launch.

Which rare events a family reaches is ASSERTED, not hoped for (family_events / require_events): a family that loses the tie digit of
some window, the most negative digit, the full carry chain or the carry-only top digit fails when it is built."""
import ctypes
import functools
import math

from oracle import bls12_381 as O

R = O.R
Z = 0xD201000000010000
LAM = Z * Z - 1                     # the eigenvalue of phi on G1: lambda^2 + lambda + 1 = r
HALF = LAM // 2
WIDTHS = tuple(range(4, 17)) + tuple(-c for c in range(4, 17))
MAX_CHUNKS_PER_BUCKET = 4096
HEAVY_MIN_CHUNKS = 17               # buckets cut into >= 17 chunks go through k_heavy_combine, 2 .. 16 through k_bucket_fold


# ------------------------------------------------------------------ the plan
def plan(c, glv=False):
    """[(offset, width)] of every window.  c > 0: bits // c + 1 windows of width c.  c < 0: the balanced plan with cmax = -c:
    ceil((bits + 1) / cmax) windows, the low n_hi = bits + 1 - nwin (cmax - 1) of them cmax wide and the others cmax - 1 (n_hi < 0: all
    narrow).  bits = 255, or 127 for the halves of the split."""
    bits = 127 if glv else 255
    if c > 0:
        return [(w * c, c) for w in range(bits // c + 1)]
    cm = -c
    nwin = -(-(bits + 1) // cm)
    n_hi = max(0, bits + 1 - nwin * (cm - 1))
    out, off = [], 0
    for w in range(nwin):
        wd = cm if w < n_hi else cm - 1
        out.append((off, wd))
        off += wd
    return out


def owned(nwin, rank, world):
    """The windows of the shard `rank` of `world`, in the order of their local indices."""
    return [w for w in range(nwin) if w % world == rank]


# ------------------------------------------------------------------ the recoding
def recode(value, pl, flip=0, with_carry=False):
    """The signed digits of the magnitude `value` >= 0 (flip = 1: of -value): d = raw + carry; d > 2^(w-1) - flip emits d - 2^w and
    carries; the digits are negated under flip.  So a digit lies in [-(2^(w-1) - 1), 2^(w-1)] either way: the tie stays positive, and
    under flip the magnitude's tie goes DOWN so that its negation is the positive tie again."""
    assert value >= 0 and flip in (0, 1)
    digits, carry = [], 0
    for off, w in pl:
        d = ((value >> off) & ((1 << w) - 1)) + carry
        if d > (1 << (w - 1)) - flip:
            d, carry = d - (1 << w), 1
        else:
            carry = 0
        digits.append(-d if flip else d)
    return (digits, carry) if with_carry else digits


def digits_of(v, pl):
    """The digits of the signed integer v: recode(|v|, flip = v < 0); sum of d_w 2^off_w == v when no carry leaves the top window."""
    return recode(abs(v), pl, 1 if v < 0 else 0)


def value_of(digits, pl, windows=None):
    return sum(digits[w] << pl[w][0] for w in (range(len(pl)) if windows is None else windows))


# ------------------------------------------------------------------ the endomorphism split
def split(k):
    """k -> (k1, k2), signed, with k1 + k2 lambda == k (mod r): k' = k - [k >= (r + 1) / 2] r, t = |k'| + floor(lambda / 2),
    q = floor(t / lambda), k2 = sign q, k1 = sign (t - q lambda - floor(lambda / 2))."""
    kp = k - R if k >= (R + 1) // 2 else k
    sign = -1 if kp < 0 else 1
    t = abs(kp) + HALF
    q = t // LAM
    return sign * (t - q * LAM - HALF), sign * q


def split_native(k):
    """cg1_glv_split (the host build of csrc/glv.h) as signed integers."""
    from curdleproofs_pie_amd import _native as N

    k1 = ctypes.create_string_buffer(16)
    k2 = ctypes.create_string_buffer(16)
    n1, n2 = ctypes.c_int(), ctypes.c_int()
    N.cg1_glv_split(k.to_bytes(32, "little"), k1, k2, ctypes.byref(n1), ctypes.byref(n2))
    a, b = int.from_bytes(k1.raw, "little"), int.from_bytes(k2.raw, "little")
    return (-a if n1.value else a), (-b if n2.value else b)


def rows_of(s, pl, glv):
    """The digit rows one scalar contributes: its own, or those of both halves of the split."""
    return [digits_of(v, pl) for v in split(s)] if glv else [recode(s, pl)]


# ------------------------------------------------------------------ the counters
def chunk_count(cnt, L0):
    if cnt == 0:
        return 0
    L = max(L0, -(-cnt // MAX_CHUNKS_PER_BUCKET))
    return -(-cnt // L)


def call_chunk_len(L0, rows, nlw, world=1, chunk_rule=True, cmax=None, rowcol_quad_max=1 << 18):
    """The chunk length a regime-A call of `rows` digit rows (2n with the split) over nlw owned windows runs with (the comments in
    plan_regime_a and above grown_chunk_len, csrc/msm_plan.h).  Three rules:
      1. the parameter, doubled while rows * nlw / 2^18 exceeds it (up to 65536);
    and, when "chunk_rule" is on and the call is not sharded,
      2. at least 10 between 2^20 and 2^21 rows x windows;
      3. between 2^21 and 2^24 rows x windows, where the lane-per-bucket tail runs (more buckets, nlw 2^(cmax - 1), than "rowcol_quad_max"):
         at least a WHOLE bucket -- its mean load rows / 2^(cmax - 1) plus eight standard deviations of a Poisson spread (the root of
         the mean) plus one, cut to an integer -- but below 2^22 rows x windows 20 at most.
    cmax (the plan's widest window) is needed from 2^21 rows x windows on, where the third rule starts."""
    e = rows * nlw
    L = L0
    while L < 65536 and (e >> 18) > L:
        L <<= 1
    if not chunk_rule or world != 1:
        return L
    if 1 << 20 <= e < 1 << 21 and L < 10:
        L = 10
    if 1 << 21 <= e < 1 << 24:
        assert cmax is not None, "the whole-bucket rule needs the plan's width"
        if (nlw << (cmax - 1)) > rowcol_quad_max:
            mean = rows / (1 << (cmax - 1))
            want = int(mean + 8.0 * math.sqrt(mean) + 1.0)
            if e < 1 << 22:
                want = min(want, 20)
            L = max(L, want)
    return L


def counts(scalars, is_identity, pl, glv=False, rank=0, world=1, L0=8, offsets=None, rows=None):
    """(entries, chunks) of one call, see the module's docstring.  offsets: the M + 1 term offsets of a batched call (every MSM has
    buckets of its own).  rows: [rows_of(s, pl, glv) for s in scalars] where the caller has them already."""
    own = owned(len(pl), rank, world)
    group = [0] * len(scalars)
    if offsets is not None:
        for j in range(len(offsets) - 1):
            for i in range(offsets[j], offsets[j + 1]):
                group[i] = j
    buckets = {}
    for i, s in enumerate(scalars):
        if is_identity[i]:
            continue
        for row in (rows[i] if rows is not None else rows_of(s, pl, glv)):
            for lw, w in enumerate(own):
                if row[w]:
                    key = (group[i], lw, abs(row[w]))
                    buckets[key] = buckets.get(key, 0) + 1
    return sum(buckets.values()), sum(chunk_count(cnt, L0) for cnt in buckets.values())


def shard_value(s, pl, glv, windows):
    """What the windows `windows` of the plan contribute to s * P, as a multiple of P mod r."""
    if glv:
        k1, k2 = split(s)
        return (value_of(digits_of(k1, pl), pl, windows) + LAM * value_of(digits_of(k2, pl), pl, windows)) % R
    return value_of(recode(s, pl), pl, windows) % R


# ------------------------------------------------------------------ the directed family
def _magnitudes(pl, top):
    """The family over a plan, as integers below 2^top; see edge_scalars."""
    full = (1 << top) - 1
    out = []
    for off, w in pl:
        field = ((1 << w) - 1) << off
        for v in (1, (1 << (w - 1)) - 1, 1 << (w - 1), (1 << (w - 1)) + 1, (1 << w) - 1):
            a = (v << off) & full
            out += [a, a | ((1 << off) - 1), a | (full & ~field)]
        out += [full & ~((1 << off) - 1), (1 << off) - 1]
    ties = sum((1 << (w - 1)) << off for off, w in pl) & full
    out += [ties, ties >> 1, ties - 1, ties + 1]
    return out


def can_hold_tie(pl, w, limit):
    """Whether window w can emit the digit 2^(width - 1) for a magnitude <= limit: every window below the last can; the last one reaches
    at most (limit >> offset) + the carry."""
    off, wd = pl[w]
    return w < len(pl) - 1 or min((limit >> off) + 1, 1 << wd) >= 1 << (wd - 1)


def family_events(values, pl):
    """What the signed integers `values` drive the recoder into: {(event, flip, window)} with the events "tie" (the digit
    +2^(width - 1)), "most negative" (-(2^(width - 1) - 1)), "carry chain" (a carry into every window from 1 to the top; window = the
    top one) and "carry-only top" (a non-zero top digit whose window holds no bit of the value)."""
    ev = set()
    for v in values:
        flip = 1 if v < 0 else 0
        mag = abs(v)
        digits, carry = recode(mag, pl, flip, with_carry=True)
        assert carry == 0 and value_of(digits, pl) == v, hex(v)
        chain, c_in = True, 0
        for w, (off, wd) in enumerate(pl):
            d = digits[w]
            assert -(1 << (wd - 1)) < d <= 1 << (wd - 1), (hex(v), w)
            if d == 1 << (wd - 1):
                ev.add(("tie", flip, w))
            if d == 1 - (1 << (wd - 1)):
                ev.add(("most negative", flip, w))
            if w and not c_in:
                chain = False
            raw = (mag >> off) & ((1 << wd) - 1)
            c_in = 1 if raw + c_in > (1 << (wd - 1)) - flip else 0
        top = len(pl) - 1
        if chain:
            ev.add(("carry chain", flip, top))
        if digits[top] and mag >> pl[top][0] == 0:
            ev.add(("carry-only top", flip, top))
    return ev


def require_events(values, pl, c, limit, flips):
    """Fails unless the family reaches, for each flip: the tie in every window that can hold it, the most negative digit in every window
    but the top one, a carry chain from window 0 to the top; for the 255-bit plans of c = 5 and 15 a non-zero carry-only top digit, and
    for c = 4, 8, 16 and every balanced plan the tie in the TOP window."""
    ev = family_events(values, pl)
    top = len(pl) - 1
    missing = []
    for flip in flips:
        for w in range(len(pl)):
            if can_hold_tie(pl, w, limit) and ("tie", flip, w) not in ev:
                missing.append(("tie", flip, w))
            if w < top and ("most negative", flip, w) not in ev:
                missing.append(("most negative", flip, w))
        if ("carry chain", flip, top) not in ev:
            missing.append(("carry chain", flip, top))
    if limit == (1 << 255) - 1:
        if c in (5, 15) and ("carry-only top", 0, top) not in ev:
            missing.append(("carry-only top", 0, top))
        if (c in (4, 8, 16) or c < 0) and ("tie", 0, top) not in ev:
            missing.append(("tie", 0, top))
    assert not missing, f"plan {c}: the family never reaches {missing}"
    return ev


@functools.lru_cache(maxsize=None)
def edge_scalars(c):
    """The directed family of the 255-bit plan c, every value < 2^255: for every window at offset o and width w the values 1, 2^(w-1) - 1,
    2^(w-1), 2^(w-1) + 1 and 2^w - 1 placed at o -- alone, with ones in every position below o, and with ones in every other position
    below bit 255 --, ones from o to bit 254, 2^o - 1; every window at its tie at once, that value >> 1, - 1 and + 1; and 0, 1, r - 1, r,
    r + 1, (r + 1) / 2, 2^254 - 1, 2^254, 2^255 - 1.  The required events are asserted."""
    pl = plan(c)
    fam = _magnitudes(pl, 255) + [0, 1, R - 1, R, R + 1, (R + 1) // 2, (1 << 254) - 1, 1 << 254, (1 << 255) - 1]
    fam = tuple(dict.fromkeys(fam))
    assert all(0 <= s < 1 << 255 for s in fam)
    require_events(fam, pl, c, (1 << 255) - 1, (0,))
    return fam


@functools.lru_cache(maxsize=None)
def edge_scalars_glv(c):
    """Scalars whose halves are the family's values: magnitudes from the same construction over the 128-position plan, a in
    [-floor(lambda / 2), lambda - floor(lambda / 2)), b >= 0, b lambda + a in [0, (r - 1) / 2]; each pair composed as s = b lambda + a,
    whose split is exactly (a, b), and as r - s, whose split is (-a, -b): every value of the family is k1 and k2 with both signs, so both
    rows run with flip = 0 and flip = 1.  Each composition and the required events of both rows are asserted."""
    pl = plan(c, True)
    # |a|, b <= floor(lambda / 2) keeps both signs of a and b itself in range.  A value of the construction beyond that (lambda / 2 is
    # 0.67 * 2^127) is not dropped -- the long carry chains are among those --: it keeps its windows below the top one, with an empty top
    # window and with the largest top-window value that stays below the bound whatever the windows below hold
    top_off = pl[-1][0]
    cap = max((HALF >> top_off) - 1, 0) << top_off
    mags = []
    for m in _magnitudes(pl, 127):
        low = m & ((1 << top_off) - 1)
        mags += [m] if m <= HALF else [low, low | cap]
    mags = list(dict.fromkeys(mags))
    assert all(0 <= m <= HALF for m in mags)
    pairs = []
    for i, m in enumerate(mags):
        b = mags[(7 * i + 3) % len(mags)]
        pairs += [(m, b), (-m, max(b, 1)), (mags[(5 * i + 1) % len(mags)], m)]
    out, halves = [], []
    for a, b in pairs:
        k = b * LAM + a
        if not (-HALF <= a < LAM - HALF and b >= 0 and 0 <= k <= (R - 1) // 2):
            continue
        assert split(k) == (a, b), hex(k)
        out.append(k)
        halves += [a, b]
        if k:
            assert split(R - k) == (-a, -b), hex(k)
            out.append(R - k)
            halves += [-a, -b]
    signs = {(a > 0, b > 0) for a, b in map(split, out) if a and b}
    assert len(signs) == 4, signs
    ev = require_events(halves, pl, c, HALF, (0, 1))
    for w, (off, wd) in enumerate(pl):                      # -2^(w-1) has no encoding: never emitted, whichever way the value is signed
        assert all(-(1 << (wd - 1)) < digits_of(v, pl)[w] for v in halves)
    assert any(e[0] == "tie" and e[1] == 0 for e in ev) and any(e[0] == "tie" and e[1] == 1 for e in ev)
    return tuple(dict.fromkeys(out))


# ------------------------------------------------------------------ chosen loads in chosen buckets
def sort_sub_bits(c, rows, param=0):
    """The partition sort's sub-bucket width ("sort_sub_bits"; 0: 7 up to 2^16 rows, else 8): at most the bucket bits, and so that a
    window has at most 128 bins."""
    bb = abs(c) - 1
    sub = min(bb, param if param else (7 if rows <= 1 << 16 else 8))
    while bb - sub > 7:
        sub += 1
    return sub


def bucket_loads(L0):
    return (1, L0 - 1, L0, L0 + 1, 2 * L0, 16 * L0, 16 * L0 + 1, 17 * L0, 4096 * L0, 4096 * L0 + 1)


def bucket_load_cases(c, L0):
    """[(label, scalars)]: scalar lists that put `cnt` entries into chosen buckets and nothing anywhere else.  A term m 2^off_w with
    m <= 2^(w-1) (and below 2^255) has exactly one non-zero digit, m, in window w.  The buckets: 1, the tie bucket 2^(w-1) (in a top
    window that holds fewer bits: its largest value), and the neighbours 2^sub and 2^sub + 1 across a bin edge of the sort; in the first,
    a middle and the top window.  Loads up to 17 L0 fill all those buckets in one call; the two loads at the 4096-chunk edge go one
    bucket (the tie bucket) per call.  The last case fills the heavy list to its bound, see heavy_list_case."""
    pl = plan(c)
    cases = []
    wins = (0, len(pl) // 2, len(pl) - 1)
    for cnt in bucket_loads(L0):
        if cnt == 0:
            continue
        big = cnt >= 4096 * L0
        sub = sort_sub_bits(c, (1 if big else 12) * cnt)
        per_window = []
        for w in wins:
            off, wd = pl[w]
            top = min(1 << (wd - 1), ((1 << 255) - 1) >> off)
            ms = [top] if big else [m for m in dict.fromkeys((1, top, 1 << sub, (1 << sub) + 1)) if m <= top]
            per_window.append([m << off for m in ms])
        if big:
            cases += [(f"load {cnt}, window {w}", vals * cnt) for w, vals in zip(wins, per_window)]
        else:
            cases.append((f"load {cnt}", [v for vals in per_window for v in vals] * cnt))
    for label, sc in cases:
        assert all(0 < s < 1 << 255 and sum(1 for d in recode(s, pl) if d) == 1 for s in sc[: 16]), label
    return cases


def mixed_load_case(c, L0):
    """One call in which k_bucket_fold and k_heavy_combine both have work, in the first, a middle and the top window: 2 L0 and 16 L0
    entries (2 and 16 chunks: folded) beside 16 L0 + 1 and 17 L0 (17 chunks: combined) in neighbouring buckets.  Alone, a 17-chunk bucket
    leaves the fold pass switched off (no bucket of 2 .. 16 chunks), so that the two kernels' thresholds never meet."""
    pl = plan(c)
    sc = []
    for w in (0, len(pl) // 2, len(pl) - 1):
        off, wd = pl[w]
        top = min(1 << (wd - 1), ((1 << 255) - 1) >> off)
        for m, cnt in ((1, 2 * L0), (2, 16 * L0 + 1), (3, 16 * L0), (top, 17 * L0)):
            sc += [m << off] * cnt
    assert all(0 < s < 1 << 255 for s in sc)
    return sc


def heavy_list_case(c, L0, world):
    """(scalars, rank 0's owned windows): every non-empty bucket of the shard holds exactly 16 L0 + 1 entries -- the fewest that make it
    heavy -- and every term has a non-zero digit in every owned window, so that the call's heavy buckets number exactly
    rows * nlw // (16 L0), the bound ensure() sizes the heavy list from (before its two spare slots).  That needs fewer than 16 L0 heavy
    buckets, hence a shard (world > 1) at chunk length 1."""
    pl = plan(c)
    own = owned(len(pl), 0, world)
    k = max(1, (16 * L0 - 1) // len(own))                   # distinct scalars: k * nlw heavy buckets
    scalars = []
    for j in range(k):
        s = 0
        for w in own:
            off, wd = pl[w]
            s |= (1 + (j + w) % min((1 << (wd - 1)) - 1, (((1 << 255) - 1) >> off) or 1)) << off
        assert s < 1 << 255 and all((d != 0) == (w in own) for w, d in enumerate(recode(s, pl))), (c, j)
        scalars.append(s)
    assert len(set(scalars)) == k
    rows, nlw, heavy = k * (16 * L0 + 1), len(own), k * len(own)
    for w in own:                                          # distinct scalars never share a bucket
        assert len({recode(s, pl)[w] for s in scalars}) == k, (c, w)
    assert heavy == rows * nlw // (16 * L0), (heavy, rows, nlw)
    return scalars * (16 * L0 + 1), own
