"""Every sponge position through the device's transcript engines.  Needs an MI355X.

The three kernels behind cg1_merlin_batch_device (block program, byte machine, one lane at a time) run the probe program of
tests/transcript_sweep.py at all 166 pad lengths on 70 rows (two waves, the second partial): every lane's outputs and 208-byte state
against the host transcript, lanes 0 and 69 against the plain-Python model as well.  tests/test_transcript_sweep.py ties the host
transcript to the model over the same sweep and proves from the model's trace that the sweep puts the rate boundary at every byte of
every operation.

The five device prover chains enter their first transcript step at whatever position the caller's transcript has: each runs from 166
transcripts whose prefixes put that position at 0..165, against the argument's host-driven path (the product's rounds with the host
transcript) -- proof bytes and final state."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

import merlin_model as MM
import transcript_sweep as TS

LANES = 70
MODEL_LANES = (0, 69)
FORMS = {"block program": (1, 1, 2), "byte machine": (0, 1, 1), "one lane at a time": (0, 0, 0)}      # merlin_rows, merlin_sync, cg1_merlin_last_kernel


@pytest.fixture(scope="module")
def M(native_lib):
    import curdleproofs_pie_amd.merlin as m

    return m


@pytest.fixture(scope="module")
def swept(M):
    """Per pad: the program, 70 rows of different data, the host transcript's (outputs, 208-byte state) for every row and the model's
    (outputs, 203 state bytes) for rows 0 and 69.  Computed once; the three kernel forms read it."""
    out = {}
    for L in TS.PADS:
        prog, plan, nbytes = TS.probe_program(M, L)
        rows = [TS.seeded_row(k, nbytes) for k in range(LANES)]
        host = []
        for row in rows:
            t = M.CurdleproofsTranscript(TS.LABEL)
            o = TS._run(t, plan, row, prog.out_bytes, lambda t, lab: bytes(t.get_and_append_challenge(lab).to_le_bytes()))
            host.append((TS.drawn(plan, o), bytes(t.strobe._st.raw)))
        model = {}
        for k in MODEL_LANES:
            o, st = TS.run_model(plan, rows[k], prog.out_bytes)
            model[k] = (TS.drawn(plan, o), st)
            assert (host[k][0], host[k][1][:203]) == model[k], (L, k)        # (the CPU test's link, on these rows)
        out[L] = dict(prog=prog, plan=plan, rows=rows, host=host, model=model)
    return out


@pytest.mark.parametrize("form", list(FORMS))
def test_batch_kernels_at_every_pad(native_lib, swept, form):
    ctx = native_lib.default_context()
    rows_param, sync_param, kernel = FORMS[form]
    ctx.set_param("merlin_rows", rows_param)
    ctx.set_param("merlin_sync", sync_param)
    try:
        for L, s in swept.items():
            prog = s["prog"]
            assert TS.run_emulator(prog, s["rows"][0]) is not None, "pad %d: refused by the row format" % L
            outs, states = prog.run(s["rows"], want_states=True)
            assert native_lib.cg1_merlin_last_kernel(ctx.handle) == kernel, (L, "fell back to another kernel")
            assert len(outs) == len(states) == LANES
            for k in range(LANES):
                assert TS.drawn(s["plan"], outs[k]) == s["host"][k][0], (form, L, k)
                assert states[k] == s["host"][k][1], (form, L, k)
            for k in MODEL_LANES:
                assert (TS.drawn(s["plan"], outs[k]), states[k][:203]) == s["model"][k], (form, L, k)
    finally:
        ctx.set_param("merlin_rows", 1)
        ctx.set_param("merlin_sync", 1)


# ------------------------------------------------------------------------------------------------ the entry step of each prover chain
def golden_cases(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)["cases"]


def entry_transcripts(k):
    """166 transcripts of a fixture case whose prefixes are L = 0..165 seeded bytes: the chain's first step starts at every position."""
    ts = [k.transcript(prefix=TS.seeded_row(1000 + L, L)) for L in TS.PADS]
    assert {bytes(t.strobe._st.raw)[200] for t in ts} == set(range(MM.RATE))
    return ts


def check(T, got, ts_dev, want, ts_host):
    assert len(got) == len(want) == MM.RATE
    for L in TS.PADS:
        assert T.to_bytes(got[L]) == T.to_bytes(want[L]), ("proof bytes", L)
        assert T.state(ts_dev[L]) == T.state(ts_host[L]), ("transcript state", L)
    assert len({T.state(t) for t in ts_dev}) == MM.RATE


def comp(pts):
    return [bytes(p.to_compressed_bytes()) for p in pts]


def ipa_host_driven_many(T, table, prover, ts):
    """test_ipa_device_gpu.host_driven for one prover's inputs under many transcripts, the rounds in step (ipa_rounds_many): the blinder
    commitments do not depend on the transcript and are computed once."""
    from curdleproofs_pie_amd.prover_kernels import ipa_rounds_many

    G, Gp, H, C, D, z, c, d, rc, rd = prover[:10]
    k = prover[10] if len(prover) > 10 else None
    B_c, B_d = table.msm_many([(G, rc), (Gp, rd if k is None else [a * b for a, b in zip(rd, k)])])
    jobs, gammas = [], []
    for t in ts:
        t.append_list(b"ipa_step1", comp([C, D]))
        t.append(b"ipa_step1", T.fr32(z))
        t.append_list(b"ipa_step1", comp([B_c, B_d]))
        alpha = t.get_and_append_challenge(b"ipa_alpha")
        beta = t.get_and_append_challenge(b"ipa_beta")
        jobs.append((G, Gp, H, [r + alpha * x for r, x in zip(rc, c)], [r + alpha * x for r, x in zip(rd, d)], k, beta))

        def next_gamma(L_C, L_D, R_C, R_D, t=t):
            t.append_list(b"ipa_loop", comp([L_C, L_D, R_C, R_D]))
            return t.get_and_append_challenge(b"ipa_gamma")

        gammas.append(next_gamma)
    return [(B_c, B_d) + tuple(r) for r in ipa_rounds_many(jobs, gammas, table=table)]


@pytest.mark.parametrize("shape", ["fixture", "all zero"])
def test_ipa_chain_entered_at_every_position(native_lib, shape):
    """n = 8.  "all zero": C, D, B_c, B_d and every L / R are the identity, absorbed from the chain's constant block and not from the row."""
    import test_ipa_device_gpu as T
    from curdleproofs_pie_amd import Scalar
    from curdleproofs_pie_amd.prover_kernels import ipa_prove_device_many

    k = T.Case(golden_cases("ipa_device_vectors.json")[1])
    assert k.n == 8
    try:
        prover = k.prover()
        if shape == "all zero":
            zero = [Scalar(0)] * k.n
            ident = k.table.msm(zero, k.G)
            prover = (k.G, k.Gp, k.H, ident, ident, Scalar(0), zero, zero, zero, zero)
        ts_dev, ts_host = entry_transcripts(k), entry_transcripts(k)
        got = ipa_prove_device_many(k.table, [prover] * MM.RATE, ts_dev)
        want = ipa_host_driven_many(T, k.table, prover, ts_host)
        check(T, got, ts_dev, want, ts_host)
        if shape == "all zero":
            inf = b"\xc0" + bytes(47)
            assert T.to_bytes(got[0])[:48 * 14] == inf * 14
    finally:
        k.table.close()


def test_same_msm_chain_entered_at_every_position(native_lib):
    """n = 8: three calls (64 provers at the most per call)."""
    import test_same_msm_device_gpu as T
    from curdleproofs_pie_amd.msm_accumulator import compute_MSM_batch
    from curdleproofs_pie_amd.prover_kernels import same_msm_prove_device_many, same_msm_rounds_many

    k = T.Case(golden_cases("same_msm_device_vectors.json")[1])
    assert k.n == 8 and native_lib.SAME_MSM_MAX_PROVERS == 64
    try:
        prover = k.prover()
        G, A, Z_t, Z_u, Tv, U, x, r = (list(v) if isinstance(v, (list, tuple)) else v for v in prover)
        ts_dev, ts_host = entry_transcripts(k), entry_transcripts(k)
        got = same_msm_prove_device_many(k.table, [prover] * MM.RATE, ts_dev)
        # test_same_msm_device_gpu.host_driven under many transcripts, the rounds in step: the three B's do not depend on the transcript
        B = compute_MSM_batch([(G, r), (Tv, r), (U, r)])
        jobs, gammas = [], []
        for t in ts_host:
            t.append_list(b"same_msm_step1", comp([A, Z_t, Z_u]))
            t.append_list(b"same_msm_step1", comp(Tv + U))
            t.append_list(b"same_msm_step1", comp(B))
            alpha = t.get_and_append_challenge(b"same_msm_alpha")
            jobs.append((G, Tv, U, [ri + alpha * xi for ri, xi in zip(r, x)]))

            def next_gamma(*pts, t=t):
                t.append_list(b"same_msm_loop", comp(pts))
                return t.get_and_append_challenge(b"same_msm_gamma")

            gammas.append(next_gamma)
        want = [tuple(B) + tuple(res) for res in same_msm_rounds_many(jobs, gammas)]
        check(T, got, ts_dev, want, ts_host)
    finally:
        k.table.close()


def test_grand_product_chain_entered_at_every_position(native_lib):
    """(ell, blinders) = (4, 4), n = 8."""
    import test_grand_product_device_gpu as T
    from curdleproofs_pie_amd.prover_kernels import grand_product_prove_device_many

    k = T.Case(golden_cases("grand_product_device_vectors.json")[3])
    assert (k.ell, k.nb) == (4, 4)
    try:
        prover = k.prover()
        ts_dev, ts_host = entry_transcripts(k), entry_transcripts(k)
        got = grand_product_prove_device_many(k.table, [prover] * MM.RATE, ts_dev)
        want = [T.host_driven(k.table, *prover, t) for t in ts_host]
        check(T, got, ts_dev, want, ts_host)
    finally:
        k.table.close()


def test_same_permutation_chain_entered_at_every_position(native_lib):
    """(ell, blinders) = (4, 4), n = 8.  This chain's own first step -- A, M, vec_a, the alpha and beta draws -- runs on the HOST transcript
    inside the call (gprod_chain's head, csrc/capi_gprod.h); the device takes over at gprod_step1, at a position the beta draw has fixed.
    So what moves with the entry position here is host code, and a fault in the device's sponge cannot show in this test."""
    import test_same_permutation_device_gpu as T
    from curdleproofs_pie_amd.prover_kernels import same_permutation_prove_device_many

    k = T.Case(golden_cases("same_permutation_device_vectors.json")[3])
    assert (k.ell, k.nb) == (4, 4)
    try:
        prover = k.prover()
        ts_dev, ts_host = entry_transcripts(k), entry_transcripts(k)
        got = same_permutation_prove_device_many(k.table, [prover] * MM.RATE, ts_dev)
        want = [T.host_driven(k.table, *prover, t) for t in ts_host]
        check(T, got, ts_dev, want, ts_host)
    finally:
        k.table.close()


def test_same_scalar_chain_entered_at_every_position(native_lib):
    """The smallest fixture case (ell = 1): three calls (64 provers at the most per call)."""
    import test_same_scalar_device_gpu as T
    from curdleproofs_pie_amd.prover_kernels import same_scalar_prove_device_many

    k = T.Case(golden_cases("same_scalar_device_vectors.json")[0])
    assert k.ell == 1 and native_lib.SAME_SCALAR_MAX_PROVERS == 64
    try:
        prover = k.prover()
        ts_dev, ts_host = entry_transcripts(k), entry_transcripts(k)
        got = same_scalar_prove_device_many(k.table, [prover] * MM.RATE, ts_dev)
        want = [T.host_driven(*prover, t) for t in ts_host]
        check(T, got, ts_dev, want, ts_host)
    finally:
        k.table.close()
