"""Every sponge position through the host-side transcript engines, without a GPU.

tests/merlin_model.py (plain Python, one byte at a time) is first pinned to what the repository holds from the reference; then the probe
program of tests/transcript_sweep.py runs at all 166 pad lengths through the host transcript (csrc/merlin.cpp), the block-program emulator
(build_block_program's node tables walked on the CPU) and the grouped host path (cg1m::Group, csrc/merlin_group.h, through
cg1_merlin_group_run) -- outputs and final state, bit for bit.  The model's trace proves what the sweep reaches: every byte of every append
and of every challenge header is, at some pad, the byte that fills the rate.  The device engines: tests/test_transcript_sweep_gpu.py."""
import ctypes
import json
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import merlin_model as MM
import transcript_sweep as TS


@pytest.fixture(scope="module")
def M(native_lib):
    import curdleproofs_pie_amd.merlin as m

    return m


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(ROOT, "tests", "golden", "merlin_vectors.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------ the model, pinned
def test_model_keccak_of_the_zero_state():
    """Keccak-f[1600] of 200 zero bytes (the first lanes of the Keccak team's published test vector)."""
    st = bytearray(200)
    MM.keccak_f1600(st)
    assert st[:16].hex() == "e7dde140798f25f18a47c033f9ccd584"
    assert int.from_bytes(st[:8], "little") == 0xF1258F7940E1DDE7


def test_model_strobe_conformance():
    """The known answer of tests/test_merlin.py::test_strobe_conformance (meta-AD, AD, PRF, KEY; a 1024-byte message: six wraps)."""
    s = MM.Strobe128(b"Conformance Test Protocol")
    s.meta_ad(b"ms", False); s.meta_ad(b"g", True); s.ad(bytes([99]) * 1024, False)
    s.meta_ad(b"prf", False)
    prf = s.prf(32, False)
    assert prf.hex() == "b48e645ca17c667fd5206ba57a6a228d72d8e1903814d3f17f622996d7cfefb0"
    s.meta_ad(b"key", False); s.key(prf, False)
    s.meta_ad(b"prf", False)
    assert s.prf(32, False).hex() == "07e45cce8078cee259e3e375bb85d75610e2d1e1201c5f645045a194edd49ff8"
    with pytest.raises(AssertionError):
        s.ad(b"x", True)


def test_model_merlin_known_answer():
    t = MM.MerlinTranscript(b"test protocol")
    t.append_message(b"some label", b"some data")
    assert t.challenge_bytes(b"challenge", 32).hex() == "d5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615"


def test_model_golden_sequences(vectors):
    assert len(vectors["cases"]) >= 10
    for case in vectors["cases"]:
        t = MM.MerlinTranscript(bytes.fromhex(case["label"]))
        for op in case["ops"]:
            lab = bytes.fromhex(op["label"])
            if op["op"] == "append":
                t.append(lab, bytes.fromhex(op["msg"]))
            elif op["op"] == "u64":
                t.append_u64(lab, op["x"])
            elif op["op"] == "challenge":
                assert t.challenge_bytes(lab, op["n"]).hex() == op["out"]
            else:
                assert t.challenge_scalar(lab).hex() == op["out"]


def test_model_live_sequence(vectors):
    """The seeded sequence of tests/test_merlin.py::test_live_against_reference_package, against the same recorded answers."""
    ref = iter(vectors["live_seed5"])
    rng = random.Random(5)
    for _ in range(6):
        t = MM.MerlinTranscript(rng.randbytes(rng.randrange(0, 30)))
        for _ in range(10):
            lab = rng.randbytes(rng.randrange(1, 12))
            if rng.random() < 0.6:
                t.append_message(lab, rng.randbytes(rng.choice([0, 7, 48, 166, 333, 1000])))
            else:
                assert t.challenge_bytes(lab, rng.choice([1, 32, 200])).hex() == next(ref)
    assert next(ref, None) is None


def test_model_trace_counts_what_it_says():
    """A transcript whose position is known by hand: Merlin's construction leaves pos = 2 + 11 + 2 + 7 + 4 + 2 + 1 = 29 for a 1-byte label."""
    tr = MM.Trace()
    t = MM.MerlinTranscript(b"x", tr)
    assert t.strobe.pos == 29 and tr.events == []
    tr.begin(0)
    t.append(b"ab", bytes(MM.RATE - 29 - 10))                    # 2 + 2 + 4 + 2 + message: ends exactly on the rate
    assert t.strobe.pos == 0 and tr.events == [(0, 0, MM.RATE - 29, False)]
    tr.begin(1)
    t.append(b"", bytes(MM.RATE - 9))                            # one byte short of the rate
    tr.begin(2)
    t.challenge_bytes(b"", 4)                                    # its first header byte fills; the PRF then forces one at pos 7
    assert tr.events[1:] == [(2, 0, 1, False), (2, 0, 8, True)] and tr.prf_zero == []
    tr.begin(3)
    t.append(b"", bytes(MM.RATE - 4 - 8 - 8))
    tr.begin(4)
    t.challenge_bytes(b"", 4)                                    # its last header byte fills: no forced permutation
    assert tr.events[3:] == [(4, 0, 8, False)] and tr.prf_zero == [(4, 0)] and t.strobe.pos == 4


# ------------------------------------------------------------------------------------------------ the sweep
@pytest.fixture(scope="module")
def swept(M):
    """Per pad: the program, its plan and row 0, and the model's answer with its trace -- computed once, read by every test below."""
    out = {}
    for L in TS.PADS:
        prog, plan, nbytes = TS.probe_program(M, L)
        row = TS.seeded_row(0, nbytes)
        trace = MM.Trace()
        want = TS.run_model(plan, row, prog.out_bytes, trace=trace)
        out[L] = dict(prog=prog, plan=plan, row=row, want=want, trace=trace)
    return out


def test_host_transcript_equals_the_model_at_every_pad(M, swept):
    for L, s in swept.items():
        assert TS.run_host(M, s["plan"], s["row"], s["prog"].out_bytes) == s["want"], L


def test_block_program_emulator_equals_the_model_at_every_pad(swept):
    for L, s in swept.items():
        got = TS.run_emulator(s["prog"], s["row"])
        assert got is not None, "pad %d: refused by the row format" % L
        assert got == s["want"], L


def test_the_sweep_reaches_every_split(swept):
    """No fallback, append coverage and challenge coverage (tests/transcript_sweep.py), from the model's own trace."""
    assert all(TS.run_emulator(s["prog"], s["row"]) is not None for s in swept.values())
    appends, challenges = TS.assert_coverage({L: (s["plan"], s["trace"]) for L, s in swept.items()}, swept[0]["plan"])
    assert (appends, challenges) == (19, 6)
    # the 32 operations are the same at every pad but for the pad's length and the data offsets
    shape = lambda plan: [(op[0], op[1], op[3] if op[0] != "scalar" and not (op[0] == "append" and op[4]) else None) for op in plan]
    assert all(shape(s["plan"]) == shape(swept[0]["plan"]) and len(s["plan"]) == TS.N_OPS for s in swept.values())


# ------------------------------------------------------------------------------------------------ the grouped host path
def group_case(L):
    plan, nbytes, nout = TS.build_plan(L, TS.GROUP_SEGMENTS, split_pad=True)
    return plan, [TS.seeded_row(100 + k, max(1, nbytes)) for k in range(16)], nout


def test_grouped_host_transcripts_at_every_pad(M):
    """16 transcripts in step at every pad: all of them against the host transcript, two against the model.  Rejected draws (more than
    half of all draws) make the transcripts drift, so the eight-wide permutation sees partial batches on both sides of 8."""
    entries = set()
    for L in TS.PADS:
        plan, rows, nout = group_case(L)
        got = TS.run_group(plan, rows, nout)
        for k in range(16):
            assert got[k] == TS.run_host(M, plan, rows[k], nout), (L, k)
        for k in (0, 15):
            assert got[k] == TS.run_model(plan, rows[k], nout), (L, k)
        entries.add(TS.run_model(plan[:3], rows[0], nout)[1][200])           # the position at which segment 1 is entered
    assert entries == set(range(MM.RATE))


def test_grouped_host_transcripts_of_every_count(M):
    """1..16 transcripts (Group::count), at a pad that puts the first header on the boundary."""
    plan, rows, nout = group_case(131)
    want = [TS.run_host(M, plan, r, nout) for r in rows]
    for n in range(1, 17):
        assert TS.run_group(plan, rows[:n], nout) == want[:n], n


def test_grouped_entry_refuses_what_the_group_does_not_take(native_lib):
    N = native_lib

    def call(ops, n=2, label=b"t", stride=80, ostride=32):
        arr = (N.MerlinOp * max(1, len(ops)))(*ops)
        out, st = ctypes.create_string_buffer(n * ostride + 1), ctypes.create_string_buffer(16 * N.MERLIN_STATE_BYTES)
        return N.cg1_merlin_group_run(label, len(label), arr, len(ops), bytes(max(1, n) * stride), stride, out, ostride, st, n)

    def op(kind, length, label=b"l", data_off=0, out_off=0):
        o = N.MerlinOp(kind=kind, label_len=len(label), pad=0, len=length, data_off=data_off, out_off=out_off)
        ctypes.memmove(o.label, label, len(label))
        return o

    assert call([op(0, 64), op(2, 32), op(0, 0)]) == 0
    assert call([]) == 0
    for bad in ([op(0, 65)], [op(1, 32)], [op(3, 32)], [op(0, 48, data_off=40)], [op(2, 32, out_off=4)], [op(2, 16)], [op(0, 8, label=b"a\0b")]):
        assert call(bad) == N.ERR_ARG
    assert call([op(0, 8)], n=0) == N.ERR_ARG and call([op(0, 8)], n=17) == N.ERR_ARG
    assert call([op(0, 8)], label=b"a\0") == N.ERR_ARG and call([op(0, 8)], label=b"x" * 33) == N.ERR_ARG
