"""The two device provers (prover_kernels.ipa_prove_device_many, same_msm_prove_device_many) alternating on ONE FixedBaseTable: both stage
their launch chain in the table handle's one staging block (csrc/capi_chain.h), which every call lays out afresh.  The calls below make
the block shrink, grow (n = 32 forces the regrow) and change layout between the two arguments; n = 2 is the smallest chain (one round,
the final scalars written straight after the first fold).  Every call must give the reference's bytes and transcript state
(tests/golden/ipa_device_vectors.json, same_msm_device_vectors.json), whatever the call before left behind.  Needs an MI355X."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu


def P(h):
    from curdleproofs_pie_amd.py_arkworks_bls12381 import G1Point
    return G1Point.from_compressed_bytes_unchecked(bytes.fromhex(h))


def S(h):
    from curdleproofs_pie_amd.py_arkworks_bls12381 import Scalar
    return Scalar.from_le_bytes(bytes.fromhex(h))


def fr32(s):
    return bytes(s.to_le_bytes())


def proof_bytes(res):
    """IPA.to_bytes / SameMSMProof.to_bytes: the points and vectors of points in the result's order, then the final scalars."""
    out = b""
    for f in res:
        for v in f if isinstance(f, list) else [f]:
            out += bytes(v.to_compressed_bytes()) if hasattr(v, "to_compressed_bytes") else fr32(v)
    return out


def transcript(case, prefix=None):
    from curdleproofs_pie_amd.merlin import CurdleproofsTranscript

    t = CurdleproofsTranscript(case["label"].encode())
    t.append(case["prefix_label"].encode(), bytes.fromhex(case["prefix"]) if prefix is None else prefix)
    return t


def ipa_prover(case):
    assert case["form"] == "explicit"
    vec = lambda key: [S(h) for h in case[key]]
    return ([P(h) for h in case["crs_G_vec"]], [P(h) for h in case["crs_G_prime_vec"]], P(case["crs_H"]), P(case["C"]), P(case["D"]), S(case["z"]),
            vec("vec_c"), vec("vec_d"), vec("vec_r_c"), vec("vec_r_d"))


def same_msm_prover(case):
    vec = lambda key: [S(h) for h in case[key]]
    return ([P(h) for h in case["crs_G_vec"]], P(case["A"]), P(case["Z_t"]), P(case["Z_u"]), [P(h) for h in case["vec_T"]], [P(h) for h in case["vec_U"]],
            vec("vec_x"), vec("vec_r"))


def rotated(pr, rot):
    """Prover `rot` of a same-MSM call in step, as tests/test_same_msm_device_gpu.py makes it: rotated scalars, permuted T / U."""
    n = len(pr[6])
    r = lambda v, k: v[k % n:] + v[:k % n]
    U = r(pr[5], 2 * rot)
    return pr[:4] + (r(pr[4], rot), U[::-1] if rot % 2 else U, r(pr[6], rot), r(pr[7], 3 * rot))


def test_provers_alternate_on_one_table(native_lib):
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable
    from curdleproofs_pie_amd.prover_kernels import ipa_prove_device_many, same_msm_prove_device_many

    load = lambda name: {c["n"]: c for c in reversed(json.load(open(os.path.join(ROOT, "tests", "golden", name)))["cases"])}      # the first case of each n
    ipa_cases, smsm_cases = load("ipa_device_vectors.json"), load("same_msm_device_vectors.json")
    ipa = {n: ipa_prover(ipa_cases[n]) for n in (2, 8, 32)}
    smsm = {n: same_msm_prover(smsm_cases[n]) for n in (2, 8, 32)}
    table = FixedBaseTable([b for n in (2, 8, 32) for b in ipa[n][0] + ipa[n][1] + [ipa[n][2]] + smsm[n][0]])
    try:
        def run_ipa(n):
            t = transcript(ipa_cases[n])
            (res,) = ipa_prove_device_many(table, [ipa[n]], [t])
            assert proof_bytes(res).hex() == ipa_cases[n]["proof"], ("ipa", n)
            assert fr32(t.get_and_append_challenge(b"after")).hex() == ipa_cases[n]["after"], ("ipa", n)

        def run_smsm(n, batch=1):
            case = smsm_cases[n]
            prefix = lambda i: None if i == 0 else b"prover %d" % i
            ts = [transcript(case, prefix(i)) for i in range(batch)]
            got = same_msm_prove_device_many(table, [rotated(smsm[n], i) for i in range(batch)], ts)
            states = [bytes(t.strobe._st.raw) for t in ts]
            assert proof_bytes(got[0]).hex() == case["proof"], ("same_msm", n)
            assert fr32(ts[0].get_and_append_challenge(b"after")).hex() == case["after"], ("same_msm", n)
            return [(proof_bytes(g), s) for g, s in zip(got, states)]

        run_ipa(8)
        run_smsm(2)
        run_ipa(2)
        in_step = run_smsm(32, batch=3)
        run_ipa(32)
        run_smsm(8)
        run_ipa(8)
        for i in (1, 2):                                                 # provers 1 and 2 of the call in step: what they give alone
            t = transcript(smsm_cases[32], b"prover %d" % i)
            (res,) = same_msm_prove_device_many(table, [rotated(smsm[32], i)], [t])
            assert (proof_bytes(res), bytes(t.strobe._st.raw)) == in_step[i], i
    finally:
        table.close()
