"""Exact relations in bulk, host side: cg1_exact_relations (the twin of the device's k_exact_relations, csrc/shuffle_verify.cpp) against the
oracle's verdicts on tests/exact_relation_cases.py, its refusals, and the two single-proof entries whose arithmetic it was factored out of
-- cg1_shuffle_exact_same_scalar and cg1_opening_exact -- against the reference's verdicts and against the flat-array entry itself."""
import ctypes
import json
import os
import struct

import pytest

import exact_relation_cases as X
from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def c():
    return X.cases()


def run_host(N, points96, scalars32, terms, threads=0):
    n = len(terms) // (8 * X.TERMS)
    ok = ctypes.create_string_buffer(b"\xee" * (n + 1), n + 1)
    rc = N.cg1_exact_relations(points96, len(points96) // 96, scalars32, len(scalars32) // 32, terms, n, ok, threads)
    assert ok.raw[n:] == b"\xee"
    return rc, [bool(b) for b in ok.raw[:n]] if rc == 0 else None


@pytest.mark.parametrize("threads", [1, 0])
def test_host_twin_equals_the_oracle(native_lib, c, threads):
    assert 200 <= len(c.relations) <= 300 and len(c.terms) == 32 * len(c.relations) and all(c.events[e] for e in X.REQUIRED_EVENTS)
    assert any(p is not None and not O.g1_in_subgroup(p) for p in c.points) and None in c.points
    assert {(1 << 256) - 1, O.R, O.R - 1, 0} <= set(c.scalars)
    rc, got = run_host(native_lib, c.points96, c.scalars32, c.terms, threads)
    assert rc == 0
    wrong = [(r[0], r[1], g) for r, g in zip(c.relations, got) if g != r[3]]
    assert not wrong, wrong[:8]
    # ... and relation by relation, reversed: no verdict depends on its neighbours
    rev = b"".join(c.terms[32 * i: 32 * i + 32] for i in range(len(c.relations) - 1, -1, -1))
    assert run_host(native_lib, c.points96, c.scalars32, rev, threads) == (0, c.want[::-1])


def test_out_of_range_indices_are_refused(native_lib, c):
    N = native_lib
    npts, nsc = len(c.points), len(c.scalars)
    rec = lambda p, k: struct.pack("<II", p, k)
    none = rec(X.NONE_MARK, 0)
    good = rec(0, 0) + rec(npts - 1, (nsc - 1) | X.NEG) + rec(1, X.ONE_MARK | X.NEG) + rec(X.NONE_MARK, 0x12345678)   # an absent record's scalar is not read
    assert run_host(N, c.points96, c.scalars32, good)[0] == 0
    for bad in (rec(npts, 0), rec(npts, X.ONE_MARK), rec(0xFFFFFFFE, 0), rec(0, nsc), rec(0, nsc | X.NEG), rec(0, X.ONE_MARK - 1), rec(0x80000000, 0)):
        for pos in range(X.TERMS):
            terms = good + b"".join(bad if j == pos else none for j in range(X.TERMS))
            assert N.cg1_exact_relations_check(terms, 2, npts, nsc) == N.ERR_ARG
            assert run_host(N, c.points96, c.scalars32, terms)[0] == N.ERR_ARG
    assert N.cg1_exact_relations_check(good, 1, npts, nsc) == 0
    assert N.cg1_exact_relations_check(good, 1, npts - 1, nsc) == N.ERR_ARG and N.cg1_exact_relations_check(good, 1, npts, nsc - 1) == N.ERR_ARG
    assert N.cg1_exact_relations_check(None, 0, 0, 0) == 0 and N.cg1_exact_relations_check(None, 1, 1, 1) == N.ERR_ARG
    assert N.cg1_exact_relations_check(none * 4, 1, 0, 0) == 0                       # no term names nothing
    assert N.cg1_exact_relations_check(none * 4, 1, 1, X.ONE_MARK) == N.ERR_ARG      # an array so long that an index would read as a marker
    # a coordinate that is no field element
    assert run_host(N, (O.P).to_bytes(48, "little") + bytes(48), c.scalars32, rec(0, X.ONE_MARK) + none * 3)[0] == N.ERR_ENCODING


def test_single_proof_entries_keep_the_reference_verdicts(native_lib):
    """cg1_opening_exact and cg1_shuffle_exact_same_scalar go through the factored arithmetic: the reference's verdicts on the torsion fixture,
    and for every opening proof the same verdict from cg1_opening_challenges + cg1_exact_relations over the oracle's decoding of its points."""
    N = native_lib
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "torsion_vectors.json")))
    ok = ctypes.c_int(-1)
    gen = X.E.raw96(O.G1_GEN)
    compared = 0
    for case in t["opening"]:
        b = {k: bytes.fromhex(case[k]) for k in ("r_G", "k_r_G", "k_commitment", "proof")}
        assert N.cg1_opening_exact(b["r_G"] + b["k_r_G"], b["k_commitment"], b["proof"], ctypes.byref(ok)) == 0
        assert bool(ok.value) == case["accepts"], case["name"]
        st = ctypes.c_int(-1)
        assert N.cg1_opening_exact_status(b["r_G"] + b["k_r_G"], b["k_commitment"], b["proof"], ctypes.byref(st)) == 0
        if st.value not in (0, 6):
            continue                                        # a scalar or a point that does not decode: no relation is evaluated
        c32 = ctypes.create_string_buffer(32)
        assert N.cg1_opening_challenges(b["r_G"] + b["k_r_G"], b["k_commitment"], b["proof"], 1, c32, 1) == 0
        pts = [O.g1_decompress(e) for e in (b["r_G"], b["k_r_G"], b["k_commitment"], b["proof"][:48], b["proof"][48:96])]
        p96 = gen + b"".join(X.E.raw96(p) if p is not None else bytes(96) for p in pts)
        sc = b["proof"][96:128] + c32.raw                   # s, c
        # s G + c k_G - A ; s r_G + c k_r_G - B   (opening.py:73-74)
        terms = X.pack_terms([[(1, 0, 0), (1, 1, 3), (-1, X.ONE, 4), None], [(1, 0, 1), (1, 1, 2), None, (-1, X.ONE, 5)]])
        rc, got = run_host(N, p96, sc, terms)
        assert rc == 0 and all(got) == case["accepts"], case["name"]
        compared += 1
    assert compared >= 6
    from curdleproofs_pie_amd.shuffle_verifier import ShuffleCrs

    crs = ShuffleCrs(bytes.fromhex(t["shuffle"]["crs"]))
    for case in t["shuffle"]["cases"]:
        inst = bytes.fromhex(case["pre_r"] + case["pre_k"] + case["post_r"] + case["post_k"])
        assert N.cg1_shuffle_exact_same_scalar(crs.handle, inst, bytes.fromhex(case["proof"]), ctypes.byref(ok)) == 0
        assert bool(ok.value) == case["accepts"], case["name"]
