"""The two arithmetic layers everything else rests on, at their limb and carry edges, on a machine with no GPU:

  * csrc/fp_row.h cannot be compiled for the host (it is DPP code), so its overflow analysis runs on tests/rowlane_model.py, a bit-exact
    model that asserts wherever the C++ would wrap: every Montgomery product of row_add and row_dbl at the largest operands its own
    call site admits.  tests/test_field_edges_gpu.py holds the device's limbs against the same model.
  * csrc/fr.h as compiled for the host (cg1_fr_ops_host) against Python ints over the Fr edge list, including the inputs that reach the
    branches of fr_inv_binary random scalars never reach."""
import random

import field_edge_cases as F
import rowlane_model as M

NN = (1 << 28) + 3                       # "nearly normal": what row_mul leaves in limbs 0..12 (fp_row.h)
P = M.P


def at_most(limb_max, value_max):
    """The row with limbs 0..12 at their per-limb maxima and the top limb as large as keeps the value <= value_max."""
    low = list(limb_max) if isinstance(limb_max, (list, tuple)) else [limb_max] * 13
    top = (value_max - M.value(low[:13])) >> 364
    assert top >= 0
    return M.row(low[:13] + [top])


def plus(kp, x=NN):
    return [x + kp[j] for j in range(13)]


def check_product(a, b, c=None, d=None):
    stats = {}
    out = M.mul2(a, b, c, d, stats=stats)                                      # asserts inside: no accumulator, carry or limb sum wraps
    prods = [(M.value(a), M.value(b))] + ([(M.value(c), M.value(d))] if c else [])
    assert sum(x * y for x, y in prods) < P << 392                            # the value precondition of every Montgomery product here
    assert M.value(out) == M.montgomery_quotient(*prods)
    assert max(out[:13]) <= NN and out[14] == out[15] == 0
    return out, stats["acc"]


def test_row_products_hold_at_the_maxima_of_their_call_sites():
    """The analogue of t_worst_case_bounds (tests/native/fp28_harness.cpp) for rows.  Operands: limbs 0..12 at the largest value the
    stage comments of row_add / row_dbl admit, the top limb at the largest the value bound admits."""
    KP3, KP6, KP12 = M.KP[3], M.KP[6], M.KP[12]
    # ---- row_add.  Stored coordinates are nearly normal with X < 11p, Y < 5p, ZZ, ZZZ < 2p (g1_xyzz.h).
    X, Y, Z = at_most(NN, 11 * P), at_most(NN, 5 * P), at_most(NN, 2 * P)
    check_product(X, Z); check_product(Y, Z); check_product(Z, Z)             # stage 1 (U, S) and ZZ1 ZZ2, ZZZ1 ZZZ2 of stage 2
    # P = U2 + (kp3 - U1), R alike: a nearly-normal limb plus at most a whole limb of the padded 3p; value < 2p + 3p
    Pd = at_most(plus(KP3), 5 * P)
    assert max(Pd[:13]) < 3 << 28
    _, acc = check_product(Pd, Pd)                                            # stage 2: PP = P P, RR = R R
    assert acc > 9 << 56 > 1 << 59                                            # ... more than 2^59, and safe
    N2 = at_most(NN, 2 * P)                                                   # any product's result: nearly normal, < 2p
    check_product(Pd, N2); check_product(N2, N2)                              # stage 3: P PP | U1 PP, ZZ12 PP
    # X3 = RR + (kp3 - PPP) + 2 (kp3 - Q): at most RR + 3 kp3 per limb, then two carry passes
    x3 = M.norm_pass(M.norm_pass(M.add(M.add(N2, M.row(KP3)), [2 * v for v in M.row(KP3)])))
    assert max(x3[:13]) <= (1 << 28) + 1 and M.value(x3) == M.value(N2) + 9 * P
    # stage 4: Y3 = R (Q - X3) - S1 PPP = R qx + PPP ns1 with qx = Q + (kp12 - X3) (value < 2p + 12p), ns1 = kp3 - S1 (at most kp3)
    qx = at_most(plus(KP12), 14 * P)
    _, acc4 = check_product(Pd, qx, N2, M.row(KP3))
    check_product(N2, N2, [0] * 16, [0] * 16)                                 # row 3 of the same stage: ZZZ3 = ZZZ12 PPP + 0 0
    # ---- row_dbl.  U = 2 Y: limbs <= 2 NN, value < 10p;  M = 3 XX: limbs <= 3 NN, value < 6p
    U, Mx = at_most(2 * NN, 10 * P), at_most(3 * NN, 6 * P)
    check_product(U, U); check_product(X, X)                                  # stage 1: V, XX
    check_product(U, N2); check_product(X, N2); check_product(N2, Z)          # stage 2: W = U V, S = X V, ZZ3 = V ZZ
    _, accm = check_product(Mx, Mx)                                           #          MM = M M
    x3 = M.norm_pass(M.norm_pass(M.add(N2, [2 * v for v in M.row(KP3)])))    # X3 = MM + 2 (kp3 - S)
    assert max(x3[:13]) <= (1 << 28) + 1
    sx = at_most(plus(KP12), 14 * P)                                          # stage 3: Y3 = M sx + W ny, ny = kp6 - Y (at most kp6)
    _, acc3 = check_product(Mx, sx, N2, M.row(KP6))
    check_product(N2, Z, [0] * 16, [0] * 16)                                  #          ZZZ3 = W ZZZ + 0 0
    # what fp_row.h states: max(a) max(b) + max(c) max(d) <= 13 * 2^56 is enough (and every call site is below it)
    for a, b, c, d in ((Pd, Pd, None, None), (Mx, Mx, None, None), (Pd, qx, N2, M.row(KP3)), (Mx, sx, N2, M.row(KP6))):
        lim = max(a[:13]) * max(b[:13]) + (max(c[:13]) * max(d[:13]) if c else 0)
        assert lim <= 13 << 56
    assert max(acc, acc4, accm, acc3) < 13 << 56


def test_row_products_at_the_stated_limb_bound():
    """The contract fp_row.h states for row_mul / row_mul2 -- max(a) max(b) + max(c) max(d) <= 13 * 2^56 -- taken at equality."""
    lim = 13 << 56
    big = int(lim ** 0.5)
    assert big * big <= lim < (big + 1) * (big + 1)
    a = M.row([big] * 13 + [0])
    assert M.value(a) ** 2 < P << 392
    check_product(a, a)
    half = int((lim // 2) ** 0.5)
    h = M.row([half] * 13 + [0])
    check_product(h, h, h, h)


def test_row_model_matches_big_integers_on_carry_edges():
    """Values and limb bounds of the model over the operand classes the device test uses (random, all-ones, nearly normal, ripple)."""
    rng = random.Random(5)
    full = (1 << 28) - 1
    edge = [M.row([full] * 13 + [0x1A011]), M.row([NN] * 13 + [0x1A011]), M.row([1 << 28] * 13 + [0x1A011]),
            M.row([1 << 28] + [full] * 12 + [0x1A011]), M.row(M.limbs_of(1)), M.row(M.limbs_of(P - 1)), M.row(M.D_R1), M.row(M.D_P)]
    rows = edge + [M.row([rng.randrange(NN + 1) for _ in range(13)] + [rng.randrange(0x34000)]) for _ in range(200)]
    for i, a in enumerate(rows):
        b = rows[(7 * i + 3) % len(rows)]
        check_product(a, b)
        check_product(a, b, rows[(5 * i + 1) % len(rows)], rows[(3 * i + 2) % len(rows)])
    # the ripple: one carry walks through all 13 limbs in ONE pass only if each pass may add it to an all-ones limb
    t = M.norm_pass(M.row([1 << 28] + [full] * 12 + [5]))
    assert t[:14] == [0, 1 << 28] + [full] * 11 + [5] and M.value(t) == M.value([1 << 28] + [full] * 12 + [5])


def test_row_add_and_dbl_chains_stay_in_bounds():
    """The whole of row_add / row_dbl on the model -- every lazy subtraction checked limb by limb, every product checked for wrap -- over
    nearly-normal coordinates at their admitted values (random operands are not points: only magnitudes matter here; the device test
    checks the group law).  Results are stored coordinates again: nearly normal, X < 11p, the others < 2p."""
    rng = random.Random(6)
    for trial in range(40):
        def coord(vmax, hi=trial % 2 == 0):
            low = [NN if hi else rng.randrange(NN + 1) for _ in range(13)]
            return at_most(low, vmax) if hi else M.row(low + [rng.randrange((vmax >> 364) - 1)])
        a = (coord(11 * P), coord(5 * P), coord(2 * P), coord(2 * P))
        b = (coord(11 * P), coord(5 * P), coord(2 * P), coord(2 * P))
        for out in (M.row_add(a, b), M.row_dbl(a)):
            assert all(max(c[:13]) <= NN and c[14] == c[15] == 0 for c in out)
            assert M.value(out[0]) < 11 * P and all(M.value(c) < 2 * P for c in out[1:])


def host(native_lib):
    return native_lib.cg1_fr_ops_host


def test_host_fr_operations_on_the_edge_list(native_lib):
    cases = F.fr_cases()
    assert sorted(cases) == list(range(10))
    for op, (ins, want) in cases.items():
        got = F.run(host(native_lib), op, F.items(ins))
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (op, i, [hex(v) for v in ins[i]], hex(g[0]), hex(w[0]))


def test_inversion_inputs_reach_every_branch_of_the_binary_inverse(native_lib):
    """fr_inv_binary ends with `for (; e > eb; --e)`, taken only when its loop ran k = 255, 256 or 257 steps; random scalars give
    k = 333..395.  The edge list must reach each of those, a long run (k >= 500) and the random range -- counted by a replay of the loop --
    and there both inversions must give pow(a, -1, r)."""
    r = F.R_MOD
    ks = {a: F.inv_binary_k(a) for a in F.fr_edges() if a}
    assert {ks[1], ks[2], ks[4]} == {255, 256, 257} and ks[3] == 256 and ks[1 << 254] >= 500
    seen = set(ks.values())
    assert {255, 256, 257} <= seen and max(seen) >= 500 and any(333 <= k <= 395 for k in seen)
    assert all(255 <= k <= 510 for k in seen)
    pick = [a for a, k in ks.items() if k <= 257 or k >= 500]
    for op in (F.OP_INV, F.OP_INV_BINARY):
        got = F.run(host(native_lib), op, F.items([(a, 0) for a in pick]))
        for a, (g, ok) in zip(pick, got):
            assert g == pow(a, -1, r) * F.R2 % r and g * a % r == F.R2, (op, hex(a), ks[a])
