"""The provers of the inner-product and the same-MSM arguments in plain Python, written from the protocol's equations (the comments of
csrc/ipa_rounds.h and csrc/same_msm_rounds.h state every term) and from nothing in the product: Python integers mod r, the transcript of
tests/merlin_model.py, and a group that is a parameter.

The model folds the BASES every round (G <- G_L + gamma G_R), as the protocol is written.  The kernels never do: they keep a coefficient
per original index over bases that stay where they are.  That difference is what makes the two independent readings of one protocol.

Two groups:
  OraclePoints   a point is an affine pair of oracle/bls12_381.py (None: the identity); MSMs and scalings through oracle/c_oracle.py.
                 Exact and slow: n point scalings per fold.
  DiscreteLogs   every base is g * G and is held as the integer g mod r; additions and scalings are integer arithmetic, and a point
                 exists only when it is emitted, O.g1_compress(O.g1_mul(G, g)).  A proof of n = 2048 costs its 46 emitted points.

A prover takes the bases and vectors, the blinders (inputs, as for the device entries), the encodings it only hashes, and a transcript
(`transcript(label, prefix_label, prefix)`); it returns a Proof: the bytes in the reference's to_bytes order, the challenges, every
intermediate vector, and `after` = get_and_append_challenge(b"after"), which pins the transcript's final state."""
from oracle import bls12_381 as O
from oracle import c_oracle as C

from merlin_model import MerlinTranscript

R = O.R
INF = b"\xc0" + bytes(47)


def transcript(label, prefix_label=None, prefix=None):
    t = MerlinTranscript(label)
    if prefix_label is not None:
        t.append_message(prefix_label, prefix)
    return t


def inner(a, b):
    return sum(x * y for x, y in zip(a, b)) % R


class OraclePoints:
    """Elements: affine pairs of the oracle, None for the identity."""

    @staticmethod
    def _raw(p):
        return bytes(96) if p is None else p[0].to_bytes(48, "little") + p[1].to_bytes(48, "little")

    @staticmethod
    def _pt(raw):
        return None if raw == bytes(96) else (int.from_bytes(raw[:48], "little"), int.from_bytes(raw[48:], "little"))

    def add(self, a, b):
        return O.g1_add(a, b)

    def mul(self, a, k):
        return self._pt(C.scalar_mul(self._raw(a), (k % R).to_bytes(32, "little")))

    def msm(self, bases, scalars):
        n = len(bases)
        return self._pt(C.compute_msm(b"".join(self._raw(p) for p in bases), b"".join((s % R).to_bytes(32, "little") for s in scalars), n))

    def encode(self, a):
        return O.g1_compress(a)


class DiscreteLogs:
    """Elements: g mod r, standing for g * G.  Encodings are remembered: a pool of bases that repeats is encoded once."""

    def __init__(self):
        self._enc = {0: INF}

    def add(self, a, b):
        return (a + b) % R

    def mul(self, a, k):
        return a * k % R

    def msm(self, bases, scalars):
        return inner(bases, scalars)

    def encode(self, a):
        a %= R
        if a not in self._enc:
            self._enc[a] = O.g1_compress(O.g1_mul(O.G1_GEN, a))
        return self._enc[a]


class Proof:
    def __init__(self, names):
        self.names, self.parts, self.challenges, self.rounds = names, {}, {}, []

    def finish(self, t):
        self.proof = b"".join(self.parts[k] for k in self.names)
        self.after = t.challenge_scalar(b"after")
        return self


def _scalar(t, label):
    return int.from_bytes(t.challenge_scalar(label), "little")


def ipa_slots(n):
    lg = n.bit_length() - 1
    return ["B_c", "B_d"] + ["%s[%d]" % (v, r) for v in ("L_C", "R_C", "L_D", "R_D") for r in range(lg)] + ["c_final", "d_final"]


def same_msm_slots(n):
    lg = n.bit_length() - 1
    return ["B_a", "B_t", "B_u"] + ["%s[%d]" % (v, r) for v in ("L_A", "L_T", "L_U", "R_A", "R_T", "R_U") for r in range(lg)] + ["x_final"]


def first_difference(names, got, want):
    """The name of the first proof slot in which two byte strings differ (None: equal).  Points take 48 bytes, the scalars 32."""
    at = 0
    for name in names:
        size = 32 if name.endswith("_final") else 48
        if got[at: at + size] != want[at: at + size]:
            return name
        at += size
    return None if len(got) == len(want) == at else "length"


def ipa_prove(grp, G, Gp, H, C48, D48, z, vec_c, vec_d, vec_r_c, vec_r_d, t):
    """<c, d> = z with C = <c, G>, D = <d, G'>: blind with alpha, then halve.  G' is given as group elements: a caller with the
    coefficient form passes G'[j] = coeff[j] * base[j]."""
    n = len(vec_c)
    assert n >= 2 and n & (n - 1) == 0 and len(G) == len(Gp) == len(vec_d) == len(vec_r_c) == len(vec_r_d) == n
    out = Proof(ipa_slots(n))
    G, Gp = list(G), list(Gp)
    B_c, B_d = grp.msm(G, vec_r_c), grp.msm(Gp, vec_r_d)
    out.parts["B_c"], out.parts["B_d"] = grp.encode(B_c), grp.encode(B_d)
    for item in (C48, D48, (z % R).to_bytes(32, "little"), out.parts["B_c"], out.parts["B_d"]):
        t.append_message(b"ipa_step1", item)
    alpha, beta = _scalar(t, b"ipa_alpha"), _scalar(t, b"ipa_beta")
    c = [(r + alpha * x) % R for r, x in zip(vec_r_c, vec_c)]
    d = [(r + alpha * x) % R for r, x in zip(vec_r_d, vec_d)]
    out.challenges.update(alpha=alpha, beta=beta, gammas=[])
    out.blinded = (list(c), list(d))
    Hb = grp.mul(H, beta)
    k = 0
    while n > 1:
        n //= 2
        cL, cR, dL, dR = c[:n], c[n:], d[:n], d[n:]
        GL, GR, GpL, GpR = G[:n], G[n:], Gp[:n], Gp[n:]
        four = (grp.add(grp.msm(GR, cL), grp.mul(Hb, inner(cL, dR))), grp.msm(GpL, dR),
                grp.add(grp.msm(GL, cR), grp.mul(Hb, inner(cR, dL))), grp.msm(GpR, dL))
        for name, p in zip(("L_C", "L_D", "R_C", "R_D"), four):
            out.parts["%s[%d]" % (name, k)] = grp.encode(p)
            t.append_message(b"ipa_loop", out.parts["%s[%d]" % (name, k)])
        gamma = _scalar(t, b"ipa_gamma")
        gamma_inv = pow(gamma, -1, R)
        c = [(a + gamma_inv * b) % R for a, b in zip(cL, cR)]
        d = [(a + gamma * b) % R for a, b in zip(dL, dR)]
        G = [grp.add(a, grp.mul(b, gamma)) for a, b in zip(GL, GR)]
        Gp = [grp.add(a, grp.mul(b, gamma_inv)) for a, b in zip(GpL, GpR)]
        out.challenges["gammas"].append(gamma)
        out.rounds.append(dict(points=four, c=list(c), d=list(d)))
        k += 1
    out.parts["c_final"], out.parts["d_final"] = c[0].to_bytes(32, "little"), d[0].to_bytes(32, "little")
    out.finals = (c[0], d[0])
    return out.finish(t)


def same_msm_prove(grp, G, A48, Zt48, Zu48, T, U, vec_x, vec_r, t, encoded_TU=None):
    """A = <x, G>, Z_t = <x, T>, Z_u = <x, U> for one x: blind with alpha, then halve all three base vectors with gamma.
    encoded_TU (optional): the 2 n encodings the transcript absorbs, where the caller has them already."""
    n = len(vec_x)
    assert n >= 2 and n & (n - 1) == 0 and len(G) == len(T) == len(U) == len(vec_r) == n
    out = Proof(same_msm_slots(n))
    G, T, U = list(G), list(T), list(U)
    B = [grp.msm(V, vec_r) for V in (G, T, U)]
    for name, p in zip(("B_a", "B_t", "B_u"), B):
        out.parts[name] = grp.encode(p)
    tu = encoded_TU if encoded_TU is not None else [grp.encode(p) for p in T + U]
    assert len(tu) == 2 * n
    for item in [A48, Zt48, Zu48] + list(tu) + [out.parts[k] for k in ("B_a", "B_t", "B_u")]:
        t.append_message(b"same_msm_step1", item)
    alpha = _scalar(t, b"same_msm_alpha")
    x = [(r + alpha * v) % R for r, v in zip(vec_r, vec_x)]
    out.challenges.update(alpha=alpha, gammas=[])
    out.blinded = list(x)
    k = 0
    while n > 1:
        n //= 2
        xL, xR = x[:n], x[n:]
        six = tuple(grp.msm(V[n:], xL) for V in (G, T, U)) + tuple(grp.msm(V[:n], xR) for V in (G, T, U))
        for name, p in zip(("L_A", "L_T", "L_U", "R_A", "R_T", "R_U"), six):
            out.parts["%s[%d]" % (name, k)] = grp.encode(p)
            t.append_message(b"same_msm_loop", out.parts["%s[%d]" % (name, k)])
        gamma = _scalar(t, b"same_msm_gamma")
        gamma_inv = pow(gamma, -1, R)
        x = [(a + gamma_inv * b) % R for a, b in zip(xL, xR)]
        G, T, U = ([grp.add(a, grp.mul(b, gamma)) for a, b in zip(V[:n], V[n:])] for V in (G, T, U))
        out.challenges["gammas"].append(gamma)
        out.rounds.append(dict(points=six, x=list(x)))
        k += 1
    out.parts["x_final"] = x[0].to_bytes(32, "little")
    out.finals = (x[0],)
    return out.finish(t)
