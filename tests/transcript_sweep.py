"""The probe program of the sponge-position sweep: one operation list per pad length L = 0..165, built so that, over the 166 pads, every
byte of every operation between a variable-length message and the next challenge is once the byte that fills the 166-byte rate.

Six segments, each opening with append(b"pad", row[0:L]): a challenge leaves the sponge at a fixed position (a PRF starts a fresh block),
so the pad shifts everything up to the next challenge by L.  The data of the other appends follows the pad in the row, so its alignment
moves with L as well.

The runners here put the same plan through the plain-Python model (tests/merlin_model.py), the host transcript and the block-program
emulator; `coverage` turns the model's traces into the sets the tests assert."""
import ctypes

import merlin_model as MM

LABEL = b"sweep"
PADS = range(MM.RATE)

# (kind, label, length):  a = append from the row, s = scalar challenge, c = challenge_bytes, e = append of own output (draw, shift, length)
SEGMENTS = [
    [("a", b"ipa_step1", 48), ("a", b"ipa_step1", 48), ("a", b"ipa_step1", 32), ("a", b"ipa_step1", 48), ("a", b"ipa_step1", 48),
     ("s", b"ipa_alpha"), ("s", b"ipa_beta")],                                                        # the IPA step's own shape
    [("a", b"ipa_loop", 48)] * 4 + [("s", b"ipa_gamma")],
    [("a", b"odd", 3), ("a", b"curdleproofs_step1", 48), ("a", b"", 1), ("a", b"same_msm_step1", 200), ("a", b"nothing", 0),
     ("c", b"raw17", 17)],                                                                            # unaligned data offsets
    [("e", b"echo", "raw17", s, 13) for s in range(4)] + [("c", b"raw48", 48)],                       # four late pieces in one block
    [("e", b"echo48", "raw48", 0, 48), ("c", b"raw164", 164)],                                        # destination words 9..12; the widest squeeze
    [("s", b"last")],
]
GROUP_SEGMENTS = [SEGMENTS[0], SEGMENTS[1], SEGMENTS[5]]                                              # what the grouped host path takes
N_OPS = sum(len(s) + 1 for s in SEGMENTS)
assert N_OPS == 32


def build_plan(L, segments=SEGMENTS, split_pad=False):
    """-> (plan, data-row length, output-row length).  Plan entries: ("append", label, data_off, len, is_pad), ("scalar", label, out_off),
    ("bytes", label, out_off, len), ("echo", label, out_off, len).  split_pad: the pad as three appends of at most 64 bytes."""
    plan, off, out, draws = [], L, 0, {}
    for seg in segments:
        if split_pad:
            a, b, c = min(L, 64), min(max(L - 64, 0), 64), max(L - 128, 0)
            plan += [("append", b"pad", 0, a, True), ("append", b"pad", a, b, True), ("append", b"pad", a + b, c, True)]
        else:
            plan.append(("append", b"pad", 0, L, True))
        for op in seg:
            if op[0] == "a":
                plan.append(("append", op[1], off, op[2], False))
                off += op[2]
            elif op[0] == "s":
                plan.append(("scalar", op[1], out))
                out += 32
            elif op[0] == "c":
                draws[op[1].decode()] = out
                plan.append(("bytes", op[1], out, op[2]))
                out += (op[2] + 3) & ~3
            else:
                plan.append(("echo", op[1], draws[op[2]] + op[3], op[4]))
    return plan, off, out


def program_from_plan(M, plan, label=LABEL):
    prog = M.TranscriptProgram(label)
    for op in plan:
        if op[0] == "append":
            prog.append(op[1], op[2], op[3])
        elif op[0] == "scalar":
            assert prog.challenge_scalar(op[1]) == op[2]
        elif op[0] == "bytes":
            assert prog.challenge_bytes(op[1], op[3]) == op[2]
        else:
            prog.append_output(op[1], op[2], op[3])
    return prog


def probe_program(M, L):
    """-> (TranscriptProgram, plan, data-row length) of pad length L: 32 operations."""
    plan, nbytes, nout = build_plan(L)
    prog = program_from_plan(M, plan)
    assert len(prog._ops) == N_OPS and prog.out_bytes == nout and prog.data_bytes <= nbytes
    return prog, plan, nbytes


def _run(t, plan, row, nout, scalar, trace=None):
    out = bytearray(nout)
    for i, op in enumerate(plan):
        if trace is not None:
            trace.begin(i)
        if op[0] == "append":
            t.append(op[1], bytes(row[op[2]: op[2] + op[3]]))
        elif op[0] == "scalar":
            out[op[2]: op[2] + 32] = scalar(t, op[1])
        elif op[0] == "bytes":
            out[op[2]: op[2] + op[3]] = t.challenge_bytes(op[1], op[3])
        else:
            t.append(op[1], bytes(out[op[2]: op[2] + op[3]]))
    return bytes(out)


def run_model(plan, row, nout, label=LABEL, trace=None):
    """-> (output row, 203 state bytes) from the plain-Python model; `trace` (a merlin_model.Trace) is filled in."""
    t = MM.MerlinTranscript(label, trace)
    out = _run(t, plan, row, nout, lambda t, lab: t.challenge_scalar(lab), trace)
    return out, t.state()


def run_host(M, plan, row, nout, label=LABEL):
    """The same from the host transcript (csrc/merlin.cpp behind CurdleproofsTranscript)."""
    t = M.CurdleproofsTranscript(label)
    out = _run(t, plan, row, nout, lambda t, lab: bytes(t.get_and_append_challenge(lab).to_le_bytes()))
    return out, bytes(t.strobe._st.raw[:203])


def run_emulator(prog, row):
    """ONE transcript through the block program on the CPU -> (output row, 203 state bytes), or None when the row format refuses it."""
    from curdleproofs_pie_amd import _native as N

    row = bytes(row)
    ops = (N.MerlinOp * len(prog._ops))(*prog._ops)
    out = ctypes.create_string_buffer(max(4, prog.out_bytes))
    st = ctypes.create_string_buffer(N.MERLIN_STATE_BYTES)
    passes = ctypes.c_uint32(0)
    rc = N.cg1_merlin_block_program_emulate(prog._init, ops, len(prog._ops), row + b"\0" * 4, len(row), out, len(out), st, ctypes.byref(passes))
    if rc == N.ERR_ARG:
        return None
    assert rc == 0
    return out.raw[:prog.out_bytes], st.raw[:203]


def run_group(plan, rows, nout, label=LABEL):
    """1..16 transcripts in step through cg1m::Group (cg1_merlin_group_run) -> [(output row, 203 state bytes)] per transcript."""
    from curdleproofs_pie_amd import _native as N

    ops = []
    for op in plan:
        kind, length, doff, ooff = (0, op[3], op[2], 0) if op[0] == "append" else (2, 32, 0, op[2])
        assert op[0] in ("append", "scalar")
        o = N.MerlinOp(kind=kind, label_len=len(op[1]), pad=0, len=length, data_off=doff, out_off=ooff)
        ctypes.memmove(o.label, op[1], len(op[1]))
        ops.append(o)
    n, stride = len(rows), max(1, len(rows[0]))
    assert all(len(r) == len(rows[0]) for r in rows)
    out = ctypes.create_string_buffer(n * nout)
    st = ctypes.create_string_buffer(n * N.MERLIN_STATE_BYTES)
    data = b"".join(bytes(r).ljust(stride, b"\0") for r in rows)
    rc = N.cg1_merlin_group_run(label, len(label), (N.MerlinOp * len(ops))(*ops), len(ops), data, stride, out, nout, st, n)
    assert rc == 0, rc
    sb = N.MERLIN_STATE_BYTES
    return [(out.raw[k * nout: (k + 1) * nout], st.raw[k * sb: k * sb + 203]) for k in range(n)]


def drawn(plan, out):
    """The challenges of an output row, in order (a slot is rounded up to four bytes: what lies between two slots is nobody's)."""
    return [bytes(out[op[2]: op[2] + (32 if op[0] == "scalar" else op[3])]) for op in plan if op[0] in ("scalar", "bytes")]


def seeded_row(seed, nbytes):
    """Row `seed`: bytes that differ from row to row and from offset to offset (no zero runs that would hide a missed XOR)."""
    import random

    return random.Random(0x5EED0000 + seed).randbytes(nbytes)


def framing(op):
    """Bytes of an append or echo operation (2 + label + 4 + 2 + message) / framing bytes of a challenge (2 + label + 4 + 2)."""
    return 8 + len(op[1]) + (op[3] if op[0] in ("append", "echo") else 0)


def coverage(plans_and_traces):
    """From the model's traces over the pads: fills[(op, n)] = the pads at which byte n (1-based) of the first part of operation `op` was the
    byte that filled the sponge; zero[op] = the pads at which that operation's PRF began at pos == 0."""
    fills, zero = {}, {}
    for L, (plan, trace) in plans_and_traces.items():
        for op, part, nbytes, forced in trace.events:
            if part == 0 and not forced:
                fills.setdefault((op, nbytes), set()).add(L)
        for op, part in trace.prf_zero:
            if part == 0:
                zero.setdefault(op, set()).add(L)
    return fills, zero


def assert_coverage(plans_and_traces, plan_of):
    """The two coverage conditions, over operation indices that are the same at every pad (`plan_of`: any pad's plan).
    Append coverage: every byte of every non-pad append or echo is the filling byte at some pad.  Challenge coverage: every challenge
    that directly follows a pad has every framing byte as the filling byte at some pad, and begins its PRF at pos == 0 at some pad."""
    fills, zero = coverage(plans_and_traces)
    appends = challenges = 0
    for i, op in enumerate(plan_of):
        if op[0] in ("append", "echo") and not (op[0] == "append" and op[4]):
            appends += 1
            missing = [n for n in range(1, framing(op) + 1) if not fills.get((i, n))]
            assert not missing, (i, op[:2], missing)
    # a challenge "follows a pad" when no other challenge stands between it and the pad: its position moves with L
    moved = False
    for i, op in enumerate(plan_of):
        if op[0] == "append" and op[4]:
            moved = True
        elif op[0] in ("scalar", "bytes") and moved:
            moved = False
            challenges += 1
            missing = [n for n in range(1, framing(op) + 1) if not fills.get((i, n))]
            assert not missing, (i, op[:2], missing)
            assert zero.get(i), (i, op[:2])
            # the PRF begins at pos == 0 exactly where the last header byte was the filling one
            assert zero[i] == fills[(i, framing(op))], (i, op[:2])
    return appends, challenges
