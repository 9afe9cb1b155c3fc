"""Merlin over STROBE-128 over Keccak-f[1600] in plain Python ints and a bytearray, written from the specifications (FIPS 202 section 3 for
the permutation, the STROBE v1.0.2 paper's section 6-7 operations, Merlin's transcript framing) and from nothing in csrc/: the one reading
of the construction that has no fast path.  Every byte is absorbed or squeezed on its own, the sponge position wraps in exactly one place,
and a trace says where each permutation fell -- which operation, after how many of its bytes, forced by the operation or by a full block.

The tests hold the six transcript engines of the product against it (tests/test_transcript_sweep.py, tests/test_transcript_sweep_gpu.py)
after pinning it to the reference's recorded answers."""

RATE = 166                                                  # STROBE-128 over a 200-byte sponge: 200 - 128 / 4 - 2
FLAG_I, FLAG_A, FLAG_C, FLAG_T, FLAG_M, FLAG_K = 1, 2, 4, 8, 16, 32
FR_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001      # r of BLS12-381
_M64 = (1 << 64) - 1


def _round_constants():
    """FIPS 202 algorithm 5: rc(t) from the LFSR x^8 + x^6 + x^5 + x^4 + 1, placed at bit 2^j - 1 of round constant i."""
    out, reg = [], 1
    for _ in range(24):
        rc = 0
        for j in range(7):
            if reg & 1:
                rc |= 1 << ((1 << j) - 1)
            reg <<= 1
            if reg & 0x100:
                reg ^= 0x171
        out.append(rc)
    return out


def _rotations():
    """FIPS 202 algorithm 2: lane (x, y) rotates by (t + 1)(t + 2) / 2 along the walk (x, y) <- (y, 2x + 3y) from (1, 0).  Lanes are
    indexed x + 5 y here, as they lie in the byte string."""
    rot = [0] * 25
    x, y = 1, 0
    for t in range(24):
        rot[x + 5 * y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return rot


_RC, _RHO = _round_constants(), _rotations()
_PI = [(i // 5) + 5 * ((2 * (i % 5) + 3 * (i // 5)) % 5) for i in range(25)]      # algorithm 3: lane (x, y) moves to (y, 2x + 3y)
_CHI1 = [(i % 5 + 1) % 5 + 5 * (i // 5) for i in range(25)]                       # algorithm 4: the two lanes to the right in the row
_CHI2 = [(i % 5 + 2) % 5 + 5 * (i // 5) for i in range(25)]
assert _RC[0] == 1 and _RC[1] == 0x8082 and _RC[23] == 0x8000000080008008 and _RHO[1] == 1 and _RHO[10] == 3 and sorted(_PI) == list(range(25))


def keccak_f1600(state):
    """One permutation of a 200-byte bytearray, in place: lane (x, y) is the little-endian 64-bit word at byte 8 (x + 5 y)."""
    a = [int.from_bytes(state[8 * i: 8 * i + 8], "little") for i in range(25)]
    b = [0] * 25
    for rc in _RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]                  # theta
        d = [c[(x + 4) % 5] ^ ((c[(x + 1) % 5] << 1 | c[(x + 1) % 5] >> 63) & _M64) for x in range(5)]
        for i in range(25):                                                                          # rho and pi
            t, n = a[i] ^ d[i % 5], _RHO[i]
            b[_PI[i]] = (t << n | t >> (64 - n)) & _M64
        a = [b[i] ^ (~b[_CHI1[i]] & b[_CHI2[i]]) for i in range(25)]                                 # chi
        a[0] ^= rc                                                                                   # iota
    for i in range(25):
        state[8 * i: 8 * i + 8] = a[i].to_bytes(8, "little")


class Strobe128:
    """The subset of STROBE-128/1600 that Merlin uses (meta-AD, AD, PRF) and KEY."""

    def __init__(self, protocol_label, trace=None):
        self.st = bytearray(200)
        self.st[0:6] = bytes([1, RATE + 2, 1, 0, 1, 96])
        self.st[6:18] = b"STROBEv1.0.2"
        self.permutations = 0
        self.trace = trace                       # a Trace, or None
        keccak_f1600(self.st)
        self.pos = self.pos_begin = self.cur_flags = 0
        self.meta_ad(protocol_label, False)

    # ---- the duplex
    def _run_f(self, forced):
        self.st[self.pos] ^= self.pos_begin
        self.st[self.pos + 1] ^= 0x04
        self.st[RATE + 1] ^= 0x80
        keccak_f1600(self.st)
        self.permutations += 1
        self.pos = self.pos_begin = 0
        if self.trace is not None:
            self.trace.permutation(forced)

    def _step(self):
        self.pos += 1
        if self.trace is not None:
            self.trace.nbytes += 1
        if self.pos == RATE:
            self._run_f(False)

    def _absorb(self, data):
        for byte in data:
            self.st[self.pos] ^= byte
            self._step()

    def _overwrite(self, data):
        for byte in data:
            self.st[self.pos] = byte
            self._step()

    def _squeeze(self, n):
        out = bytearray()
        for _ in range(n):
            out.append(self.st[self.pos])
            self.st[self.pos] = 0
            self._step()
        return out

    def _begin_op(self, flags, more):
        if more:
            assert self.cur_flags == flags, "`more` must continue the same operation"
            return
        assert not flags & FLAG_T, "no transport operations here"
        old_begin = self.pos_begin
        self.pos_begin = self.pos + 1
        self.cur_flags = flags
        self._absorb(bytes([old_begin, flags]))
        if flags & (FLAG_C | FLAG_K):
            if self.pos != 0:
                self._run_f(True)
            elif self.trace is not None and flags & FLAG_I:
                self.trace.prf_at_zero()

    # ---- operations
    def meta_ad(self, data, more):
        self._begin_op(FLAG_M | FLAG_A, more)
        self._absorb(data)

    def ad(self, data, more):
        self._begin_op(FLAG_A, more)
        self._absorb(data)

    def prf(self, n, more):
        self._begin_op(FLAG_I | FLAG_A | FLAG_C, more)
        return self._squeeze(n)

    def key(self, data, more):
        self._begin_op(FLAG_A | FLAG_C, more)
        self._overwrite(data)

    def state(self):
        """The 203 bytes every engine of the product keeps: sponge, pos, pos_begin, cur_flags."""
        return bytes(self.st) + bytes([self.pos, self.pos_begin, self.cur_flags])


class Trace:
    """Where the permutations of a run fell.  The driver names the operation it is about to run (`begin`); every Merlin-level call
    inside it is a `part` (a scalar challenge has one per draw and one for the re-append).
      events      (op, part, bytes of that part absorbed or squeezed so far, forced)   one per permutation
      prf_zero    (op, part)   a PRF whose header ended exactly on a full block: the operation forced no permutation of its own"""

    def __init__(self):
        self.op, self.part, self.nbytes = -1, 0, 0
        self.events, self.prf_zero = [], []

    def begin(self, op):
        self.op, self.part, self.nbytes = op, -1, 0

    def next_part(self):
        self.part += 1
        self.nbytes = 0

    def permutation(self, forced):
        self.events.append((self.op, self.part, self.nbytes, bool(forced)))

    def prf_at_zero(self):
        self.prf_zero.append((self.op, self.part))


class MerlinTranscript:
    def __init__(self, label, trace=None):
        self.strobe = Strobe128(b"Merlin v1.0")
        self.append_message(b"dom-sep", label)
        self.trace = self.strobe.trace = trace                    # the trace starts after the construction

    def _part(self):
        if self.strobe.trace is not None:
            self.strobe.trace.next_part()

    def append_message(self, label, message):
        self._part()
        self.strobe.meta_ad(label, False)
        self.strobe.meta_ad(len(message).to_bytes(4, "little"), True)
        self.strobe.ad(message, False)

    def append_u64(self, label, x):
        self.append_message(label, x.to_bytes(8, "little"))

    def challenge_bytes(self, label, n):
        self._part()
        self.strobe.meta_ad(label, False)
        self.strobe.meta_ad(n.to_bytes(4, "little"), True)
        return bytes(self.strobe.prf(n, False))

    # ---- the Curdleproofs adaptor
    def append(self, label, item):
        self.append_message(label, item)

    def challenge_scalar(self, label):
        """32 bytes, drawn again while they are 0 or >= r as a little-endian integer; the accepted bytes go back in under the same label."""
        while True:
            out = self.challenge_bytes(label, 32)
            if 0 < int.from_bytes(out, "little") < FR_ORDER:
                self.append_message(label, out)
                return out

    def state(self):
        return self.strobe.state()
