"""shuffle_prover.ShuffleBatchProver / cg1_whisk_shuffle_front / cg1_whisk_shuffle_prove_device (csrc/capi_whisk_shuffle.h,
csrc/kernels_whisk_shuffle.h): GenerateWhiskShuffleProof from tracker bytes, for several shuffles in step.  Needs an MI355X.

The device front is held against its host twin and the CPU oracle on the fixture cases, the edge inputs and the refusals of
tests/whisk_shuffle_cases.py, alone and three provers in step; the whole call against the reference's recorded bytes
(tests/golden/shuffle_device_vectors.json: shuffle_permute_and_commit_input and CurdleProofsProof.new;
tests/golden/whisk_shuffle_prover_vectors.json: GenerateWhiskShuffleProof itself under a recorded seed); provers in step each get what
they get alone; the package's batch verifier accepts the output; a refusal of either half leaves both outputs alone; and the call
shares one table handle with the other device provers."""
import ctypes
import json
import os
import random
import sys
import types

import pytest

from oracle import bls12_381 as O

import whisk_shuffle_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu
R, NB, INF = O.R, 4, W.INF
DRAW_KEYS = ("vec_a_blinders", "vec_c_blinders", "ipa_r", "ipa_z_head", "r_t", "r_u", "r_a", "r_b", "r_k", "vec_r")


def P(h):
    from curdleproofs_pie_amd.py_arkworks_bls12381 import G1Point
    return G1Point.from_compressed_bytes_unchecked(bytes.fromhex(h) if isinstance(h, str) else h)


def S(h):
    from curdleproofs_pie_amd.py_arkworks_bls12381 import Scalar
    return Scalar.from_le_bytes(bytes.fromhex(h))


def comp(p):
    return bytes(p.to_compressed_bytes())


def fr32(s):
    return bytes(s.to_le_bytes())


@pytest.fixture(scope="module")
def cases(native_lib):
    return W.golden("shuffle_device_vectors.json")


class Case:
    """A fixture case of shuffle_device_vectors.json as the batched prover takes it: the CRS as product objects over a FixedBaseTable of
    vec_G | vec_H | H | G_t | G_u, the pre-shuffle trackers as byte pairs, the draws as Scalars."""

    def __init__(self, case, extra_bases=()):
        from curdleproofs_pie_amd.fixed_base import FixedBaseTable

        self.raw, self.ell = case, case["ell"]
        ell, n = self.ell, self.ell + NB
        if "vec_G" in case:
            pts = [P(h) for h in case["vec_G"] + case["vec_H"] + [case["H"], case["G_t"], case["G_u"]]]
            enc = [bytes.fromhex(h) for h in case["vec_R"] + case["vec_S"]]
        else:                                                            # not stored: G1 * k, the n + 3 + 2 ell scalars k the case's seed gives first
            from curdleproofs_pie_amd import G1Point, Scalar
            from curdleproofs_pie_amd.msm_accumulator import batch_mul

            rng = random.Random(case["seed"])
            count = n + 3 + 2 * ell
            every = [comp(p) for p in batch_mul([G1Point()] * count, [Scalar(rng.randint(1, R - 1)) for _ in range(count)])]
            pts, enc = [P(e) for e in every[: n + 3]], every[n + 3:]
        self.crs = types.SimpleNamespace(vec_G=pts[:ell], vec_H=pts[ell:n], H=pts[n], G_t=pts[n + 1], G_u=pts[n + 2])
        self.pre = list(zip(enc[:ell], enc[ell:]))
        self.post = [(bytes.fromhex(t), bytes.fromhex(u)) for t, u in zip(case["vec_T"], case["vec_U"])]
        self.perm, self.k = list(case["permutation"]), S(case["k"])
        self.mbl = [S(h) for h in case["vec_m_blinders"]]
        d = case["draws"]
        self.draws = tuple([S(h) for h in d[key]] if isinstance(d[key], list) else S(d[key]) for key in DRAW_KEYS)
        self.table = FixedBaseTable(pts + list(extra_bases))
        self.wire = bytes.fromhex(case["M"] + case["proof"])
        self._items = {}

    def prover(self):
        from curdleproofs_pie_amd.shuffle_prover import ShuffleBatchProver
        return ShuffleBatchProver(self.crs, table=self.table)

    def item(self, rot=0):
        """Item `rot` of a call in step: item 0 is the fixture's; the others have rotated trackers, their own k, permutation, blinders and draws."""
        from curdleproofs_pie_amd import Scalar

        if rot not in self._items:
            if rot == 0:
                it = (self.pre, self.perm, self.k, self.mbl, self.draws)
            else:
                pre = self.pre[rot % self.ell:] + self.pre[: rot % self.ell]
                if rot % 2:
                    pre = [(s, r) for r, s in pre]
                perm = list(range(self.ell))
                random.Random(1000 * self.ell + rot).shuffle(perm)
                bump = iter(range(1, 1 << 20))
                draws = tuple([s + Scalar(rot * next(bump)) for s in d] if isinstance(d, list) else d + Scalar(rot * next(bump)) for d in self.draws)
                it = (pre, perm, self.k + Scalar(rot), [b + Scalar(3 * rot + i) for i, b in enumerate(self.mbl)], draws)
            self._items[rot] = it
        return self._items[rot]


def snapshot(item):
    pre, perm, k, mbl, draws = item
    flat = lambda v: [fr32(x) for x in v] if isinstance(v, list) else fr32(v)
    return ([tuple(t) for t in pre], list(perm), fr32(k), flat(mbl), [flat(d) for d in draws])


# ---------------------------------------------------------------------------------------------------- the front
class FrontTable:
    """vec_G | vec_H of a fixture case's CRS as a table, for raw calls of the front."""

    def __init__(self, ell):
        from curdleproofs_pie_amd.fixed_base import FixedBaseTable

        self.ell = ell
        self.table = FixedBaseTable([P(e) for e in W.crs_encodings(ell)])
        self.ctxh, self.tabh = self.table._ctx.handle, self.table._tab.handle


def front(N, ft, fronts, null=(), ell=None, n_provers=None, gi=None):
    """cg1_whisk_shuffle_front on the provers `fronts` in step -> (rc, text, outputs as bytes); the outputs are pre-filled with 0xAA."""
    ell_, Pn = ft.ell, len(fronts)
    n = ell_ + NB
    u32 = lambda v: (ctypes.c_uint32 * max(1, len(v)))(*v)
    fill = lambda m: ctypes.create_string_buffer(b"\xaa" * m, m)
    out = {"rs": fill(192 * ell_ * Pn), "tu": fill(192 * ell_ * Pn), "post": fill(96 * ell_ * Pn), "m48": fill(48 * Pn)}
    raw = lambda f, key, dflt: getattr(f, "raw", {}).get(key, dflt)
    args = {"gi": u32(gi if gi is not None else list(range(ell_)) * Pn), "hi": u32(list(range(ell_, n)) * Pn), "trackers96": b"".join(f.trackers96 for f in fronts),
            "perm": u32([m for f in fronts for m in f.perm]), "k32": b"".join(raw(f, "k32", f.k32) for f in fronts),
            "mbl32": b"".join(raw(f, "mbl32", f.mbl32) for f in fronts), **out}
    for key in null:
        args[key] = None
    rc = N.cg1_whisk_shuffle_front(ft.ctxh, ft.tabh if "tab" not in null else None, ell_ if ell is None else ell, Pn if n_provers is None else n_provers, args["gi"],
                                   args["hi"], args["trackers96"], args["perm"], args["k32"], args["mbl32"], args["rs"], args["tu"], args["post"], args["m48"])
    return rc, N.cg1_ctx_error(ft.ctxh).decode(), {key: v.raw for key, v in out.items()}


def host_twin(N, f):
    """cg1_whisk_shuffle_front_emulate on one prover -> the same four outputs."""
    from curdleproofs_pie_amd.py_arkworks_bls12381 import points_to_affine96

    n = f.ell + NB
    out = {"rs": ctypes.create_string_buffer(192 * f.ell), "tu": ctypes.create_string_buffer(192 * f.ell), "post": ctypes.create_string_buffer(96 * f.ell),
           "m48": ctypes.create_string_buffer(48)}
    gh96 = bytes(points_to_affine96([P(e) for e in W.crs_encodings(f.ell)]))
    rc = N.cg1_whisk_shuffle_front_emulate(f.ell, f.trackers96, (ctypes.c_uint32 * f.ell)(*f.perm), f.k32, f.mbl32, gh96, out["rs"], out["tu"], out["post"],
                                           ctypes.create_string_buffer(32 * n), out["m48"], None)
    assert rc == N.OK, f.name
    return {key: v.raw for key, v in out.items()}


def check_front(N, ft, fronts, twin=True):
    """The device front on `fronts` in step against the oracle's records and, prover by prover, against the host twin."""
    rc, text, out = front(N, ft, fronts)
    assert rc == N.OK, text
    for key in ("rs", "tu", "post", "m48"):
        assert out[key] == b"".join(f.expected[key] for f in fronts), ([f.name for f in fronts], key)
        if twin:
            assert out[key] == b"".join(host_twin(N, f)[key] for f in fronts), ([f.name for f in fronts], key)


@pytest.mark.parametrize("which", range(3))
def test_front_reproduces_the_fixture_cases(native_lib, which):
    """ell = 4, 12, 28, one prover and three in step (the fixture's, then two with another k and permutation): the oracle's records, which
    tests/test_whisk_shuffle_prover.py holds against the host twin and the reference's vec_T, vec_U and M."""
    f, c = W.fixture_fronts()[which]
    ft = FrontTable(f.ell)
    try:
        check_front(native_lib, ft, [f])
        rc, _, out = front(native_lib, ft, [f])
        assert rc == native_lib.OK and out["m48"].hex() == c["M"]
        assert out["post"] == b"".join(bytes.fromhex(t) + bytes.fromhex(u) for t, u in zip(c["vec_T"], c["vec_U"]))
        if f.ell <= 12:                                                  # (the oracle's multiplications in Python: keep the larger case to one prover)
            rev = W.Front("reversed", f.crs, f.trackers[::-1], f.perm[1:] + f.perm[:1], f.k + 1, [b + 1 for b in f.mbl])
            swp = W.Front("swapped", f.crs, [(s, r) for r, s in f.trackers], f.perm[::-1], R - f.k, f.mbl[::-1])
            check_front(native_lib, ft, [f, rev, swp])
            check_front(native_lib, ft, [swp, f, rev])
    finally:
        ft.table.close()


def test_front_on_the_edge_inputs(native_lib):
    """Every edge input alone, then three at a time in step: a k or a perm segment indexed by the wrong prover gives another prover's bytes."""
    N = native_lib
    ft = FrontTable(4)
    try:
        edges = list(W.edge_fronts().values())
        for f in edges:
            check_front(N, ft, [f])
        for i in range(0, len(edges), 3):
            check_front(N, ft, (edges + edges)[i: i + 3], twin=False)
        check_front(N, ft, edges, twin=False)                            # all eight in step
    finally:
        ft.table.close()


def test_front_refusals_leave_the_outputs_untouched(native_lib):
    N = native_lib
    ft = FrontTable(4)
    who = "cg1_whisk_shuffle_front"
    untouched = lambda out: all(v == b"\xaa" * len(v) for v in out.values())
    try:
        edges = W.edge_fronts()
        base, others = edges["both signs"], [edges["k = 1"], edges["no bijection"]]
        check_front(N, ft, [base])
        for name, status, edit, fragments in W.refusals():
            for at, fronts in ((0, [edit(base)]), (2, others + [edit(base)]), (1, [others[0], edit(base), others[1]])):
                rc, text, out = front(N, ft, fronts)
                assert rc == getattr(N, status), (name, at, rc, text)
                assert untouched(out), (name, at)
                assert text.startswith(who + ": ") and f"prover {at}" in text, (name, text)
                for frag in fragments:
                    assert frag in text, (name, text)
                if fragments:
                    assert ("k_r_G" in text) == (fragments[1] == "k_r_G"), (name, text)
        for kw, frag in ((dict(ell=5), "power of two"), (dict(n_provers=65), "provers"), (dict(gi=[0, 1, 2, len(ft.table)]), "outside the table")):
            rc, text, out = front(N, ft, [base], **kw)
            assert rc == N.ERR_ARG and untouched(out) and text.startswith(who) and frag in text, (kw, text)
        for key in ("tab", "gi", "hi", "trackers96", "perm", "k32", "mbl32", "rs", "tu", "post", "m48"):
            rc, text, out = front(N, ft, [base], null=(key,))
            assert rc == N.ERR_ARG and untouched(out) and "bad argument" in text, key
        check_front(N, ft, [base, *others])                              # the next valid call is correct
    finally:
        ft.table.close()


# ---------------------------------------------------------------------------------------------------- the whole call
@pytest.mark.parametrize("which", range(4))
def test_fixture_cases_reproduce_reference_bytes(native_lib, cases, which):
    """ell = 4, 12, 28, 124: M || proof and the post-shuffle trackers of the reference's record, twice."""
    k = Case(cases[which])
    try:
        prover = k.prover()
        before = snapshot(k.item())
        assert native_lib.cg1_whisk_shuffle_proof_bytes(k.ell) == len(k.wire)
        first = prover.prove_many([k.item()])
        assert len(first) == 1 and first[0][0] == k.post and first[0][1] == k.wire, k.ell
        assert prover.prove_many([k.item()]) == first
        assert snapshot(k.item()) == before
    finally:
        k.table.close()


@pytest.mark.parametrize("which,batches", [(1, (1, 3, 8)), (0, (64, 70))])
def test_provers_in_step(cases, which, batches):
    """Batches of 1, 3 and 8 at ell = 12; 64 and 70 (two native calls) at ell = 4: every prover's output equals what it gets alone, all distinct."""
    k = Case(cases[which])
    try:
        prover = k.prover()
        alone = {}
        for batch in batches:
            items = [k.item(i) for i in range(batch)]
            got = prover.prove_many(items)
            assert len(got) == batch and got[0] == (k.post, k.wire)
            for i in (range(1, batch) if batch <= 8 else (1, 2, 62, 63, 64, 69)):
                if i >= batch:
                    continue
                if i not in alone:
                    alone[i] = prover.prove_many([items[i]])[0]
                assert got[i] == alone[i], (batch, i)
            assert len({proof for _, proof in got}) == batch and len({tuple(post) for post, _ in got}) == batch
    finally:
        k.table.close()


def test_generate_reproduces_the_reference_under_the_recorded_seed(native_lib):
    """GenerateWhiskShuffleProof on two lists, one after the other, as the reference ran it under random.seed(seed): both in one call,
    byte for byte, and `random` left where the reference left it."""
    from curdleproofs_pie_amd.shuffle_prover import ShuffleBatchProver, generate_whisk_shuffle_proofs

    for c in W.golden("whisk_shuffle_prover_vectors.json"):
        pts = {key: (P(c[key]) if isinstance(c[key], str) else [P(h) for h in c[key]]) for key in ("vec_G", "vec_H", "H", "G_t", "G_u", "G_sum", "H_sum")}
        crs = types.SimpleNamespace(**pts)
        lists = [[(bytes.fromhex(r), bytes.fromhex(s)) for r, s in pre] for pre in c["pre_trackers"]]
        want = [([(bytes.fromhex(r), bytes.fromhex(s)) for r, s in post], bytes.fromhex(proof)) for post, proof in zip(c["post_trackers"], c["proofs"])]
        state = random.getstate()
        try:
            with ShuffleBatchProver(crs) as prover:                      # its own table, FixedBaseTable.for_crs
                random.seed(c["seed"])
                assert prover.generate(lists) == want, c["ell"]
                assert repr(random.random()) == c["random_after"]
                rng = random.Random(c["seed"])                           # a generator of the caller's, and WhiskTracker-like objects
                assert prover.generate([[types.SimpleNamespace(r_G=r, k_r_G=s) for r, s in pre] for pre in lists], rng=rng) == want
                assert repr(rng.random()) == c["random_after"]
            random.seed(c["seed"])
            assert generate_whisk_shuffle_proofs(crs, lists) == want
        finally:
            random.setstate(state)


def crs_bytes(crs):
    from functools import reduce
    return b"".join(comp(p) for p in list(crs.vec_G) + list(crs.vec_H) + [crs.H, crs.G_t, crs.G_u, reduce(lambda a, b: a + b, crs.vec_G), reduce(lambda a, b: a + b, crs.vec_H)])


def test_the_batch_verifier_accepts(native_lib, cases):
    """A batch of 8 at ell = 28 goes into are_valid_whisk_shuffle_proofs as it comes out of prove_many; one post tracker replaced by
    another valid encoding is rejected, that item only."""
    from curdleproofs_pie_amd.shuffle_verifier import are_valid_whisk_shuffle_proofs

    k = Case(cases[2])
    try:
        items = [k.item(i) for i in range(8)]
        got = k.prover().prove_many(items)
        batch = [(it[0], post, proof) for it, (post, proof) in zip(items, got)]
        crs = crs_bytes(k.crs)
        assert are_valid_whisk_shuffle_proofs(crs, batch) == [True] * 8
        pre, post, proof = batch[3]
        r_g = bytearray(post[5][0])
        r_g[0] ^= 0x20                                                   # the other y of the same x: a valid encoding of the negated point
        assert O.g1_decompress(bytes(r_g)) == O.g1_neg(O.g1_decompress(post[5][0]))
        bad = post[:5] + [(bytes(r_g), post[5][1])] + post[6:]
        assert are_valid_whisk_shuffle_proofs(crs, batch[:3] + [(pre, bad, proof)] + batch[4:]) == [True] * 3 + [False] + [True] * 4
    finally:
        k.table.close()


def test_a_refusal_in_the_second_half_leaves_both_outputs_untouched(native_lib, cases):
    """vec_c_blinders[-2] = 0: the front succeeds, the chain refuses -- under this entry's name -- and neither output has been written."""
    from curdleproofs_pie_amd import Scalar
    from curdleproofs_pie_amd.py_arkworks_bls12381 import points_to_affine96

    N = native_lib
    k = Case(cases[1])
    ell, n = k.ell, k.ell + NB
    try:
        t, crs = k.table, k.crs
        u32 = lambda v: (ctypes.c_uint32 * max(1, len(v)))(*v)
        d = k.raw["draws"]
        vec = lambda *keys: b"".join(b"".join(bytes.fromhex(h) for h in d[key]) if isinstance(d[key], list) else bytes.fromhex(d[key]) for key in keys)
        wb = N.cg1_whisk_shuffle_proof_bytes(ell)

        def call(cbl):
            post, out = ctypes.create_string_buffer(b"\xaa" * (96 * ell), 96 * ell), ctypes.create_string_buffer(b"\xaa" * wb, wb)
            rc = N.cg1_whisk_shuffle_prove_device(t._ctx.handle, t._tab.handle, ell, 1, u32(t._indices(crs.vec_G, ell)), u32(t._indices(crs.vec_H, NB)), u32([t.index(crs.H)]),
                                                  u32([t.index(crs.G_t)]), u32([t.index(crs.G_u)]), bytes(points_to_affine96([crs.G_t, crs.G_u, crs.H])),
                                                  b"".join(r + s for r, s in k.pre), u32(k.perm), bytes.fromhex(k.raw["k"]),
                                                  b"".join(bytes.fromhex(h) for h in k.raw["vec_m_blinders"]), vec("vec_a_blinders"), cbl, vec("ipa_r"), vec("ipa_z_head"),
                                                  vec("r_t", "r_u", "r_a", "r_b", "r_k"), vec("vec_r"), post, out)
            return rc, N.cg1_ctx_error(t._ctx.handle).decode(), post.raw, out.raw

        cbl = vec("vec_c_blinders")
        rc, _, post, out = call(cbl)
        assert rc == N.OK and out == k.wire and post == b"".join(r + s for r, s in k.post)
        rc, text, post, out = call(cbl[:64] + bytes(32) + cbl[96:])
        assert rc != N.OK and text.startswith("cg1_whisk_shuffle_prove_device: "), (rc, text)
        assert post == b"\xaa" * (96 * ell) and out == b"\xaa" * wb
        # the same through the Python face: NativeError, nothing returned, and the next call is right
        item = k.item()
        zero = item[4][:1] + (item[4][1][:2] + [Scalar(0)] + item[4][1][3:],) + item[4][2:]
        prover = k.prover()
        with pytest.raises(N.NativeError):
            prover.prove_many([item, item[:4] + (zero,)])
        with pytest.raises(N.NativeError, match="prover 1: tracker 2: k_r_G"):
            prover.prove_many([item, ([*k.pre[:2], (k.pre[2][0], W.torsion_encoding()), *k.pre[3:]], *item[1:])])
        assert prover.prove_many([item]) == [(k.post, k.wire)]
    finally:
        k.table.close()
    with pytest.raises(N.NativeError):
        k.prover().prove_many([k.item()])                                # the table is closed


def test_one_table_handle_shared(native_lib, cases):
    """ipa | prove_many | whole shuffle | prove_many on ONE table handle -- one staging block, laid out afresh by every call -- each giving
    its fixture's bytes before and after."""
    from curdleproofs_pie_amd.merlin import CurdleproofsTranscript
    from curdleproofs_pie_amd.prover_kernels import ipa_prove_device, shuffle_prove_device

    def flat(res):
        out = b""
        for f in res:
            if isinstance(f, tuple):
                out += flat(f)
            else:
                for v in f if isinstance(f, list) else [f]:
                    out += comp(v) if hasattr(v, "to_compressed_bytes") else fr32(v)
        return out

    vec = lambda c, key: [S(h) for h in c[key]]
    pts = lambda c, key: [P(h) for h in c[key]]
    ipa_c = next(c for c in W.golden("ipa_device_vectors.json") if c["n"] == 8 and c.get("form") == "explicit")
    ipa = (pts(ipa_c, "crs_G_vec"), pts(ipa_c, "crs_G_prime_vec"), P(ipa_c["crs_H"]), P(ipa_c["C"]), P(ipa_c["D"]), S(ipa_c["z"]),
           vec(ipa_c, "vec_c"), vec(ipa_c, "vec_d"), vec(ipa_c, "vec_r_c"), vec(ipa_c, "vec_r_d"))
    k = Case(cases[1], extra_bases=ipa[0] + ipa[1] + [ipa[2]])
    c = k.raw
    whole = (k.crs, [P(h) for h in c["vec_R"]], [P(h) for h in c["vec_S"]], [P(h) for h in c["vec_T"]], [P(h) for h in c["vec_U"]], P(c["M"]), k.perm, k.k, k.mbl, k.draws)

    def run_ipa():
        t = CurdleproofsTranscript(ipa_c["label"].encode())
        t.append(ipa_c["prefix_label"].encode(), bytes.fromhex(ipa_c["prefix"]))
        assert flat(ipa_prove_device(k.table, *ipa, t)).hex() == ipa_c["proof"]
        assert fr32(t.get_and_append_challenge(b"after")).hex() == ipa_c["after"]

    try:
        prover = k.prover()
        run_ipa()
        assert shuffle_prove_device(k.table, *whole).hex() == c["proof"]
        assert prover.prove_many([k.item()]) == [(k.post, k.wire)]
        run_ipa()
        assert shuffle_prove_device(k.table, *whole).hex() == c["proof"]
        assert prover.prove_many([k.item(), k.item(1)])[0] == (k.post, k.wire)
    finally:
        k.table.close()
