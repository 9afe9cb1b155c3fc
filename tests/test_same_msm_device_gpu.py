"""prover_kernels.same_msm_prove_device / cg1_same_msm_prove_device (csrc/kernels_same_msm.h): the whole same-MSM argument as one launch
chain over a fixed table (crs_G_vec) and a light table built inside the call (vec_T | vec_U).  Needs an MI355X.

Pinned to the reference's bytes: tests/golden/same_msm_device_vectors.json records SameMSMProof.new run stand-alone (proof bytes, and a
challenge drawn after it that pins the final transcript state).  Provers in step must each get what they get alone; edge inputs are
compared with the host-driven path (compute_MSM_batch for the three B's, the host transcript, same_msm_rounds); every refusal leaves
the outputs and the transcript alone."""
import ctypes
import json
import os
import random
import sys

import pytest

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu
R = O.R
INF = b"\xc0" + bytes(47)


def P(h):
    from curdleproofs_pie_amd.py_arkworks_bls12381 import G1Point
    return G1Point.from_compressed_bytes_unchecked(bytes.fromhex(h) if isinstance(h, str) else h)


def S(h):
    from curdleproofs_pie_amd.py_arkworks_bls12381 import Scalar
    return Scalar.from_le_bytes(bytes.fromhex(h))


def fr32(s):
    return bytes(s.to_le_bytes())


@pytest.fixture(scope="module")
def cases(native_lib):
    return json.load(open(os.path.join(ROOT, "tests", "golden", "same_msm_device_vectors.json")))["cases"]


class Case:
    """A fixture case as product objects, with the fixed table over its crs_G_vec."""

    def __init__(self, case):
        from curdleproofs_pie_amd.fixed_base import FixedBaseTable

        self.raw, self.n = case, case["n"]
        self.G = [P(h) for h in case["crs_G_vec"]]
        self.T, self.U = [P(h) for h in case["vec_T"]], [P(h) for h in case["vec_U"]]
        self.A, self.Z_t, self.Z_u = P(case["A"]), P(case["Z_t"]), P(case["Z_u"])
        self.x, self.r = [S(h) for h in case["vec_x"]], [S(h) for h in case["vec_r"]]
        self.table = FixedBaseTable(self.G)

    def transcript(self, prefix=None):
        from curdleproofs_pie_amd.merlin import CurdleproofsTranscript

        t = CurdleproofsTranscript(self.raw["label"].encode())
        t.append(self.raw["prefix_label"].encode(), bytes.fromhex(self.raw["prefix"]) if prefix is None else prefix)
        return t

    def prover(self, rot=0):
        """Prover `rot`: rotated scalars and permuted T / U (A, Z_t, Z_u are only hashed: left as they are)."""
        r = lambda v, k: v[k % self.n:] + v[:k % self.n]
        U = r(self.U, 2 * rot)
        if rot % 2:
            U = U[::-1]
        return (self.G, self.A, self.Z_t, self.Z_u, r(self.T, rot), U, r(self.x, rot), r(self.r, 3 * rot))


def to_bytes(res):
    """SameMSMProof.to_bytes order."""
    B_a, B_t, B_u, LA, LT, LU, RA, RT, RU, x_fin = res
    return b"".join(bytes(p.to_compressed_bytes()) for p in [B_a, B_t, B_u] + LA + LT + LU + RA + RT + RU) + fr32(x_fin)


def state(t):
    return bytes(t.strobe._st.raw)


def host_driven(G, A, Z_t, Z_u, T, U, x, r, transcript):
    """SameMSMProof.new after the blinder draw, driven from the host: compute_MSM_batch, the host transcript, same_msm_rounds."""
    from curdleproofs_pie_amd.msm_accumulator import compute_MSM_batch
    from curdleproofs_pie_amd.prover_kernels import same_msm_rounds

    G, T, U, r = list(G), list(T), list(U), list(r)
    B = compute_MSM_batch([(G, r), (T, r), (U, r)])
    comp = lambda pts: [bytes(p.to_compressed_bytes()) for p in pts]
    transcript.append_list(b"same_msm_step1", comp([A, Z_t, Z_u]))
    transcript.append_list(b"same_msm_step1", comp(T + U))
    transcript.append_list(b"same_msm_step1", comp(B))
    alpha = transcript.get_and_append_challenge(b"same_msm_alpha")
    x2 = [ri + alpha * xi for ri, xi in zip(r, x)]

    def next_gamma(*pts):
        transcript.append_list(b"same_msm_loop", comp(pts))
        return transcript.get_and_append_challenge(b"same_msm_gamma")

    return tuple(B) + tuple(same_msm_rounds(G, T, U, x2, next_gamma))


@pytest.mark.parametrize("which", range(6))
def test_fixture_cases_reproduce_reference_bytes(cases, which):
    from curdleproofs_pie_amd.prover_kernels import same_msm_prove_device

    k = Case(cases[which])
    try:
        x_before = [fr32(s) for s in k.x]
        for _ in range(2):                                               # twice: the same bytes, the same state
            t = k.transcript()
            res = same_msm_prove_device(k.table, *k.prover(), t)
            assert to_bytes(res).hex() == k.raw["proof"], (k.n, k.raw["shape"])
            assert fr32(t.get_and_append_challenge(b"after")).hex() == k.raw["after"]
        assert [fr32(s) for s in k.x] == x_before                        # vec_x is not mutated
        t3 = k.transcript()                                              # the host-driven path agrees on both
        assert to_bytes(host_driven(*k.prover(), t3)).hex() == k.raw["proof"]
        assert state(t3) != state(k.transcript())
        assert fr32(t3.get_and_append_challenge(b"after")).hex() == k.raw["after"]
    finally:
        k.table.close()


@pytest.mark.parametrize("which", [1, 2, 4])
def test_provers_in_step(cases, which):
    """Batches of 1, 3, 8 and 64 provers at n = 8 (both shapes) and n = 32: rotated vectors, permuted T / U, different transcript
    prefixes; prover 0 is the fixture's; every prover's bytes and final state equal what it gets alone."""
    from curdleproofs_pie_amd.prover_kernels import same_msm_prove_device_many

    k = Case(cases[which])
    assert k.n in (8, 32)
    try:
        alone = {}
        for batch in (1, 3, 8, 64):
            provers = [k.prover(rot=i) for i in range(batch)]
            prefix = lambda i: None if i == 0 else b"prover %d" % i
            ts = [k.transcript(prefix(i)) for i in range(batch)]
            got = same_msm_prove_device_many(k.table, provers, ts)
            assert len(got) == batch
            assert to_bytes(got[0]).hex() == k.raw["proof"] and fr32(ts[0].get_and_append_challenge(b"after")).hex() == k.raw["after"]
            for i in range(1, batch):
                if i not in alone:
                    t1 = k.transcript(prefix(i))
                    alone[i] = (to_bytes(same_msm_prove_device_many(k.table, [provers[i]], [t1])[0]), state(t1))
                assert (to_bytes(got[i]), state(ts[i])) == alone[i], (batch, i)
            assert len({to_bytes(g) for g in got}) == batch
    finally:
        k.table.close()


def test_edge_inputs_against_the_host_driven_path(native_lib):
    """Seeded inputs at n = 16: x and r all zero (identity outputs, absorbed as C0 00 ..), T = U, T_i = -T_j, identities in T and U,
    a T entry outside G1 and one equal to the order-3 point t3, small scalars -- the device chain and the host-driven path give the
    same bytes and the same transcript."""
    from curdleproofs_pie_amd import G1Point, Scalar
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.merlin import CurdleproofsTranscript
    from curdleproofs_pie_amd.prover_kernels import same_msm_prove_device

    rng = random.Random(8001)
    tors = json.load(open(os.path.join(ROOT, "tests", "golden", "torsion_vectors.json")))
    T3 = O.g1_decompress(bytes.fromhex(tors["t3"]))
    assert not O.g1_in_subgroup(T3) and O.g1_mul(T3, 3) is None
    n = 16
    obj = lambda p: G1Point.from_compressed_bytes_unchecked(O.g1_compress(p))
    rpt = lambda: O.g1_mul(O.G1_GEN, rng.randrange(1, R))
    G = [obj(rpt()) for _ in range(n)]
    tab = FixedBaseTable(G)
    rs = lambda: [Scalar(rng.randrange(R)) for _ in range(n)]
    zero = [Scalar(0)] * n
    small = lambda: [Scalar(rng.randrange(4)) for _ in range(n)]
    Tp, Up = [rpt() for _ in range(n)], [rpt() for _ in range(n)]
    neg = list(Tp)
    neg[3], neg[9], neg[10] = O.g1_neg(neg[7]), neg[2], O.g1_neg(neg[2])                 # T_3 = -T_7, T_9 = T_2, T_10 = -T_2
    ids_t, ids_u = list(Tp), list(Up)
    for j in (0, 5, 12, 13, 15):
        ids_t[j] = None
    for j in (5, 6, 12, 14, 15):
        ids_u[j] = None
    tor = list(Tp)
    tor[4], tor[11] = O.g1_add(T3, tor[4]), T3                                            # order 3 r (outside G1); t3 itself
    tor_u = list(Up)
    tor_u[11] = O.g1_neg(T3)
    shapes = {
        "all zero": (Tp, Up, zero, zero),
        "T = U": (Tp, Tp, rs(), rs()),
        "opposite and equal entries": (neg, Up, rs(), rs()),
        "identities": (ids_t, ids_u, rs(), rs()),
        "all identities": ([None] * n, [None] * n, rs(), rs()),
        "torsion": (tor, tor_u, rs(), rs()),
        "torsion, small scalars": (tor, tor_u, small(), small()),
        "small scalars": (Tp, Up, small(), small()),
        "zero blinders": (Tp, Up, rs(), zero),
    }
    try:
        for name, (Tv, Uv, x, r) in shapes.items():
            T, U = [obj(p) for p in Tv], [obj(p) for p in Uv]
            A, Z_t, Z_u = tab.msm(x, G), obj(None), obj(None)                            # only hashed
            mk = lambda: CurdleproofsTranscript(b"edge " + name.encode())
            t_dev, t_host = mk(), mk()
            got = same_msm_prove_device(tab, list(range(n)), A, Z_t, Z_u, T, U, x, r, t_dev)    # bases as indices here, as objects there
            want = host_driven(G, A, Z_t, Z_u, T, U, x, r, t_host)
            assert to_bytes(got) == to_bytes(want), name
            assert state(t_dev) == state(t_host), name
            if name in ("all zero", "all identities"):                                   # every output over T | U (and, all zero, over G) is the identity
                which = range(9) if name == "all zero" else (1, 2, 4, 5, 7, 8)
                pts = [p for q in which for p in (got[q] if isinstance(got[q], list) else [got[q]])]
                assert len(pts) >= 6 and all(bytes(p.to_compressed_bytes()) == INF for p in pts), name
    finally:
        tab.close()


def raw_args(k, P_=1):
    """The C entry's arguments for P_ copies of a fixture case."""
    from curdleproofs_pie_amd.py_arkworks_bls12381 import points_to_affine96

    n = k.n
    gi = (ctypes.c_uint32 * (n * P_))(*(list(range(n)) * P_))
    azz = (bytes.fromhex(k.raw["A"]) + bytes.fromhex(k.raw["Z_t"]) + bytes.fromhex(k.raw["Z_u"])) * P_
    vec = lambda key: b"".join(bytes.fromhex(h) for h in k.raw[key]) * P_
    return dict(gi=gi, azz=azz, tu=bytes(points_to_affine96(k.T + k.U)) * P_, x=vec("vec_x"), r=vec("vec_r"))


def call_raw(N, ctx_handle, tab_handle, n, P_, a, st, out):
    return N.cg1_same_msm_prove_device(ctx_handle, tab_handle, n, P_, a["gi"], a["azz"], a["tu"], a["x"], a["r"], st, out, None)


def test_refusals_leave_everything_untouched(native_lib, cases):
    from curdleproofs_pie_amd.prover_kernels import same_msm_prove_device, same_msm_prove_device_many

    N = native_lib
    k = Case(cases[1])                                                    # n = 8, random points
    n, pb = k.n, 1040
    try:
        ctxh, tabh = k.table._ctx.handle, k.table._tab.handle
        start = state(k.transcript())

        def refused(want, n_=n, P_=1, **edit):
            a = raw_args(k, P_)
            a.update(edit)
            st = ctypes.create_string_buffer(start * P_, 208 * P_)
            out = ctypes.create_string_buffer(b"\xaa" * (pb * P_), pb * P_)
            rc = call_raw(N, ctxh, tabh, n_, P_, a, st, out)
            assert (rc == want if want is not None else rc != N.OK), (edit.keys(), rc)
            assert out.raw == b"\xaa" * (pb * P_) and st.raw == start * P_

        def good():
            a = raw_args(k)
            st = ctypes.create_string_buffer(start, 208)
            out = ctypes.create_string_buffer(pb)
            assert call_raw(N, ctxh, tabh, n, 1, a, st, out) == N.OK
            assert out.raw.hex() == k.raw["proof"] and st.raw != start

        good()
        for bad_n in (0, 1, 3, 6, 2 * N.SAME_MSM_MAX_N):
            refused(N.ERR_ARG, n_=bad_n)
        refused(N.ERR_ARG, P_=N.SAME_MSM_MAX_PROVERS + 1)
        good()
        refused(N.ERR_ARG, gi=(ctypes.c_uint32 * n)(*([0] * (n - 1) + [len(k.table)])))
        refused(N.ERR_ARG, gi=(ctypes.c_uint32 * n)(*([0] * (n - 1) + [1 << 31])))               # no negated bases here
        for key in ("x", "r"):
            for bad in (R, (1 << 256) - 1):
                buf = bytearray(raw_args(k)[key])
                buf[-32:] = bad.to_bytes(32, "little")
                refused(N.ERR_ENCODING, **{key: bytes(buf)})
        good()
        tu = raw_args(k)["tu"]
        refused(None, tu=tu[:96 * 3] + O.P.to_bytes(48, "little") + tu[96 * 3 + 48:])            # a T coordinate >= p (either byte order: p itself)
        refused(None, tu=tu[:96 * 3] + b"\xff" * 48 + tu[96 * 3 + 48:])
        refused(N.ERR_NOT_ON_CURVE, tu=tu[:96 * (n + 2)] + tu[96 * (n + 3): 96 * (n + 3) + 48] + tu[96 * (n + 2) + 48:])   # U_2 with U_3's x: off the curve
        azz = raw_args(k)["azz"]
        refused(N.ERR_ENCODING, azz=bytes([azz[0] & 0x7F]) + azz[1:])                            # A without the compression flag
        refused(N.ERR_ENCODING, azz=azz[:48] + b"\x9f" + b"\xff" * 47 + azz[96:])                # Z_t with x >= p
        off_curve = next(x for x in range(1, 50) if pow((x ** 3 + 4) % O.P, (O.P - 1) // 2, O.P) != 1)
        refused(N.ERR_NOT_ON_CURVE, azz=azz[:96] + bytes([0x80 | (off_curve >> 376)]) + off_curve.to_bytes(48, "big")[1:])
        good()
        # ---- the Python face: refusals raise and leave the caller's transcript alone
        t = k.transcript()
        pr = k.prover()
        with pytest.raises(ValueError):
            same_msm_prove_device(k.table, k.G[:6], k.A, k.Z_t, k.Z_u, k.T[:6], k.U[:6], k.x[:6], k.r[:6], t)
        with pytest.raises(ValueError):
            same_msm_prove_device(k.table, k.G[:1], k.A, k.Z_t, k.Z_u, k.T[:1], k.U[:1], k.x[:1], k.r[:1], t)
        with pytest.raises(KeyError):
            same_msm_prove_device(k.table, k.G[:-1] + [P(k.raw["crs_G_vec"][-1])], *pr[1:], t)
        with pytest.raises(IndexError):
            same_msm_prove_device(k.table, list(range(n - 1)) + [len(k.table)], *pr[1:], t)
        with pytest.raises(N.NativeError):
            same_msm_prove_device(k.table, k.G, k.A, k.Z_t, k.Z_u, k.T, k.U, k.x[:-1] + [R], k.r, t)       # a plain int >= r
        with pytest.raises(N.NativeError):
            same_msm_prove_device(k.table, k.G, b"\x00" * 48, k.Z_t, k.Z_u, k.T, k.U, k.x, k.r, t)
        with pytest.raises(ValueError):
            same_msm_prove_device_many(k.table, [pr], [])
        assert state(t) == start
        assert to_bytes(same_msm_prove_device(k.table, *pr, t)).hex() == k.raw["proof"]                    # the next valid call is correct
        assert fr32(t.get_and_append_challenge(b"after")).hex() == k.raw["after"]
        assert same_msm_prove_device_many(k.table, [], []) == []
    finally:
        k.table.close()
    with pytest.raises(N.NativeError):
        same_msm_prove_device(k.table, *k.prover(), k.transcript())                                       # the table is closed
