"""Prover-side hot loops of the shuffle argument, re-cut for the GPU.

The reference prover spends its time in four patterns, all written as Python loops over single `G1Point` operators:

  * the halving rounds of the inner-product argument       ipa.py:117-151      4 MSMs of h terms + 2 folds of h points per round
  * the halving rounds of the same-MSM argument            same_msm.py:93-130  6 MSMs of h terms + 3 folds of h points per round
  * `shuffle_permute_and_commit_input`                     curdleproofs.py:301-321   2 ell same-scalar multiplications + 2 MSMs
  * the grand-product base change G'_i = G_i * beta^-(i+1) grand_prod.py:64-71 ell + 4 per-index multiplications

Here every halving round is ONE batched GPU MSM call (`compute_MSM_batch`: a handful of small MSMs ride one k_msm_small launch) and
NO fold of the bases at all -- the round challenges are folded into the scalars instead (see ipa_rounds_many) -- and the map patterns
are one `batch_mul*` launch each.  The `*_many` forms run several independent provers in step: round k of ALL of them is still one
MSM call (cross-proof batching; tools/gpu_prover_bench.py measures both).  The Fiat-Shamir
transcript stays with the caller, exactly where the reference has it: the round functions take a `next_gamma` callback that
receives the round's commitments (to absorb them) and returns the challenge.  Scalars follow the reference's update order, so
the outputs are the same group elements / field elements the reference prover produces (tests/test_prover_kernels_gpu.py
replays inputs recorded from the reference prover and compares every L / R point and final scalar).
"""
from __future__ import annotations

import ctypes
from typing import Callable, List, Sequence, Tuple

from .msm_accumulator import batch_mul, batch_mul_same_scalar, compute_MSM, compute_MSM_batch
from .py_arkworks_bls12381 import CURVE_ORDER, G1Point, Scalar, pack_scalars
from .util import random_scalar

N_BLINDERS = 4                                                          # curdleproofs.py:24


def _inner(a: Sequence[Scalar], b: Sequence[Scalar]) -> Scalar:          # util.py:85-87
    acc = 0
    for x, y in zip(a, b):
        acc += x._v * y._v
    return Scalar(acc)


def _halves(n0: int, n: int):
    """Original indices whose CURRENT position (j mod 2n, after the halvings so far) lies in the left / right half of a vector of length 2n."""
    left = [j for j in range(n0) if j % (2 * n) < n]
    right = [j for j in range(n0) if j % (2 * n) >= n]
    return left, right


def ipa_rounds_many(provers: Sequence[Tuple[Sequence[G1Point], Sequence[G1Point], G1Point, Sequence[Scalar], Sequence[Scalar]]],
                    next_gammas: Sequence[Callable[[G1Point, G1Point, G1Point, G1Point], Scalar]], table=None):
    """ipa.py:117-151 for SEVERAL independent provers in step (same vector length): round k of all of them is ONE batched MSM call
    (4 MSMs per prover; up to 16 MSMs ride one k_msm_small launch).  provers[p] = (crs_G_vec, crs_G_prime_vec, H, vec_c, vec_d) with
    `H` = crs_H * beta (ipa.py:110) and the vectors already blinded (ipa.py:107-109).
    -> per prover (vec_L_C, vec_R_C, vec_L_D, vec_R_D, c_final, d_final).

    The reference folds the BASES every round (G = G_L + gamma G_R, ipa.py:142-146: h scalar multiplications, a 255-doubling chain
    each).  The prover never outputs a folded base -- only MSMs over them -- and a folded base is a fixed combination of the original
    ones, G^(k)_i = sum over j = i (mod n_k) of coef_j G_j with coef_j the product of the challenges of the rounds in which j sat in
    the right half.  So the bases stay what they were (normal forms cached, or resident on the device) and the challenges fold into
    the SCALARS: MSM(G^(k)_R, c_L) = sum over j in the right half of c_L[j mod 2n - n] coef_j G_j.  Same group elements, no fold
    launches at all (they were 15.8 of the 21 ms these rounds took: profiles/r03_prover_flows_v2.txt).

    table (a fixed_base.FixedBaseTable): the four MSMs of a round, for all provers in step, go through ONE `table.msm_many` call -- no
    doublings, the sums finished on the device.  Every G[j], Gp[j] and H must then be an object of the table (KeyError otherwise).
    `H` = crs_H * beta is not a CRS point: a seventh tuple element gives it implicitly, H = provers[p][2] * provers[p][6] (pass crs_H
    itself and beta), the way the sixth stands for the base change of G'; the inner-product scalars are multiplied by it instead."""
    st = [dict(G=list(pr[0]), Gp=list(pr[1]), H=pr[2], c=[x._v for x in pr[3]], d=[x._v for x in pr[4]], LC=[], RC=[], LD=[], RD=[],
               kGp0=(list(pr[5]) if len(pr) > 5 and pr[5] is not None else None),
               kH=(pr[6]._v if len(pr) > 6 and pr[6] is not None else None)) for pr in provers]
    n0 = n = len(st[0]["c"])
    assert all(len(s["c"]) == len(s["d"]) == len(s["G"]) == len(s["Gp"]) == n for s in st) and n & (n - 1) == 0
    for s in st:
        # coef_j of G_j / G'_j.  A sixth tuple element gives the G' vector implicitly: G'_j = Gp[j] * coeffs[j] -- the grand-product
        # argument's base change G'_i = G_i beta^-(i+1) (grand_prod.py:64-71) then costs no scalar multiplication at all: pass the
        # CRS points themselves as Gp and the powers as coefficients
        s["kG"], s["kGp"] = [1] * n0, ([1] * n0 if s["kGp0"] is None else [v._v for v in s["kGp0"]])
        assert len(s["kGp"]) == n0
    R = CURVE_ORDER
    S = Scalar._raw
    while n > 1:
        n //= 2
        left, right = _halves(n0, n)
        jobs = []
        for s in st:
            c, d, kG, kGp, G, Gp = s["c"], s["d"], s["kG"], s["kGp"], s["G"], s["Gp"]
            ip_l = sum(c[i] * d[n + i] for i in range(n)) % R            # <c_L, d_R>
            ip_r = sum(c[n + i] * d[i] for i in range(n)) % R            # <c_R, d_L>
            if s["kH"] is not None:                                      # H stands for H * kH
                ip_l, ip_r = ip_l * s["kH"] % R, ip_r * s["kH"] % R
            # L_C = MSM(G_R, c_L) + H <c_L, d_R>;  L_D = MSM(G'_L, d_R);  R_C = MSM(G_L, c_R) + H <c_R, d_L>;  R_D = MSM(G'_R, d_L)
            jobs += [([G[j] for j in right] + [s["H"]], [S(c[j % (2 * n) - n] * kG[j] % R) for j in right] + [S(ip_l)]),
                     ([Gp[j] for j in left], [S(d[n + j % (2 * n)] * kGp[j] % R) for j in left]),
                     ([G[j] for j in left] + [s["H"]], [S(c[n + j % (2 * n)] * kG[j] % R) for j in left] + [S(ip_r)]),
                     ([Gp[j] for j in right], [S(d[j % (2 * n) - n] * kGp[j] % R) for j in right])]
        res = compute_MSM_batch(jobs) if table is None else table.msm_many(jobs)
        for i, (s, ng) in enumerate(zip(st, next_gammas)):
            L_C, L_D, R_C, R_D = res[4 * i: 4 * i + 4]
            s["LC"].append(L_C); s["RC"].append(R_C); s["LD"].append(L_D); s["RD"].append(R_D)
            gamma = ng(L_C, L_D, R_C, R_D)._v
            gamma_inv = pow(gamma, -1, R)
            c, d, kG, kGp = s["c"], s["d"], s["kG"], s["kGp"]
            s["c"] = [(c[i] + gamma_inv * c[n + i]) % R for i in range(n)]
            s["d"] = [(d[i] + gamma * d[n + i]) % R for i in range(n)]
            for j in right:                                              # G_L[i] + G_R[i] * gamma,  G'_L[i] + G'_R[i] * gamma^-1
                kG[j] = kG[j] * gamma % R
                kGp[j] = kGp[j] * gamma_inv % R
    return [(s["LC"], s["RC"], s["LD"], s["RD"], S(s["c"][0]), S(s["d"][0])) for s in st]


def ipa_rounds(crs_G_vec: Sequence[G1Point], crs_G_prime_vec: Sequence[G1Point], H: G1Point, vec_c: Sequence[Scalar],
               vec_d: Sequence[Scalar], next_gamma: Callable[[G1Point, G1Point, G1Point, G1Point], Scalar],
               G_prime_coeffs: Sequence[Scalar] = None, H_coeff: Scalar = None, table=None):
    """ipa.py:117-151.  `H` is crs_H * beta (ipa.py:110); vec_c / vec_d are the blinded vectors (after ipa.py:107-109).
    G_prime_coeffs (optional): crs_G_prime_vec[j] stands for crs_G_prime_vec[j] * G_prime_coeffs[j] (see ipa_rounds_many).
    H_coeff (optional): `H` stands for H * H_coeff (pass crs_H and beta).  table (optional): a FixedBaseTable holding every base.
    -> (vec_L_C, vec_R_C, vec_L_D, vec_R_D, c_final, d_final)."""
    return ipa_rounds_many([(crs_G_vec, crs_G_prime_vec, H, vec_c, vec_d, G_prime_coeffs, H_coeff)], [next_gamma], table=table)[0]


def _chain_provers(provers: Sequence[tuple], transcripts: Sequence, vec_at: int, what: str, max_n: int):
    """The head of a *_prove_device_many call: -> (the provers as tuples, their vector length n = len(provers[0][vec_at]); 0 for none)."""
    provers = [tuple(pr) for pr in provers]
    if len(provers) != len(transcripts):
        raise ValueError("one transcript per prover")
    n = len(provers[0][vec_at]) if provers else 0
    if provers and (n < 2 or n & (n - 1) or n > max_n):
        raise ValueError(f"the vectors of {what} argument have a power-of-two length in 2 .. {max_n}, not {n}")
    return provers, n


def _pack32(vals: Sequence[Scalar]):
    b = ctypes.create_string_buffer(32 * max(1, len(vals)))
    pack_scalars(vals, ctypes.addressof(b), len(vals))
    return b


def _chain_prove(table, provers: Sequence[tuple], transcripts: Sequence, n: int, step: int, wrong_table: str, prove, n_points: int, n_vecs: int,
                 n_scalars: int) -> List[tuple]:
    """The frame of a *_prove_device_many call: under the table's context lock, `step` provers per chain (more provers than one chain
    carries: several calls), prove(lo, part, states) -> (proofs, new states) with the transcripts' states packed and moved back, and each
    proof's bytes cut into n_points points, n_vecs vectors of lg n points and n_scalars trailing scalars."""
    from . import _native as N

    S, lg = N.MERLIN_STATE_BYTES, n.bit_length() - 1
    out: List[tuple] = []
    with table._ctx_lock():
        if table._KIND != "fixed-base":                                  # a LightTable: its records are not what the chain's MSM kernel reads
            raise TypeError(wrong_table)
        for lo in range(0, len(provers), step):
            part, ts = provers[lo: lo + step], transcripts[lo: lo + step]
            proofs, new_states = prove(lo, part, b"".join(bytes(t.strobe._st.raw[:S]) for t in ts))
            pb = len(proofs) // len(part)
            for i, t in enumerate(ts):
                ctypes.memmove(t.strobe._st, new_states[S * i: S * i + S], S)
                raw = proofs[pb * i: pb * i + pb]
                P48 = [G1Point.from_compressed_bytes_unchecked(raw[48 * j: 48 * j + 48]) for j in range(n_points + n_vecs * lg)]
                vecs = [P48[n_points + q * lg: n_points + (q + 1) * lg] for q in range(n_vecs)]
                tail = raw[pb - 32 * n_scalars:]
                out.append((*P48[:n_points], *vecs, *(Scalar.from_le_bytes(tail[32 * k: 32 * k + 32]) for k in range(n_scalars))))
    return out


def ipa_prove_device_many(table, provers: Sequence[tuple], transcripts: Sequence) -> List[tuple]:
    """IPA.new (ipa.py:75-153) after its blinder draw, for SEVERAL independent provers of one vector length in step, proved ON THE DEVICE:
    one launch chain (csrc/kernels_ipa.h), one wait -- the MSMs over the resident `table` (a fixed_base.FixedBaseTable), the
    transcript, gamma^-1 and the folds between them never come back to the host.
    provers[p] = (crs_G_vec, crs_G_prime_vec, crs_H, C, D, z, vec_c, vec_d, vec_r_c, vec_r_d[, G_prime_coeffs]): bases are objects of the
    table or indices into it (KeyError / IndexError, FixedBaseTable._indices); C, D are G1Points or their 48-byte encodings (only
    hashed); z and the vectors are Scalars, vec_c / vec_d UNBLINDED (the call blinds them with the alpha it draws) and the blinders
    the caller's own (the reference's generate_ipa_blinders, ipa.py:27-48); G_prime_coeffs as in ipa_rounds_many.
    transcripts[p]: that prover's CurdleproofsTranscript, advanced to the state after the last ipa_gamma -- the caller goes on exactly
    where the reference would.  -> per prover (B_c, B_d, vec_L_C, vec_R_C, vec_L_D, vec_R_D, c_final, d_final), the fields of IPA.
    A refused call (ValueError: n not a power of two >= 2; NativeError: a scalar >= r, an undecodable C or D) changes nothing."""
    from . import _native as N
    from .py_arkworks_bls12381 import points_to_compressed

    provers, n = _chain_provers(provers, transcripts, 6, "an inner-product", N.IPA_MAX_N)
    if not provers:
        return []
    if any(not (len(pr[0]) == len(pr[1]) == len(pr[6]) == len(pr[7]) == len(pr[8]) == len(pr[9]) == n) for pr in provers):
        raise ValueError("provers in step share one vector length")
    coeffs = [pr[10] if len(pr) > 10 else None for pr in provers]
    if any(k is not None and len(k) != n for k in coeffs):
        raise ValueError("G_prime_coeffs has one entry per base")
    enc = iter(points_to_compressed([x for pr in provers for x in pr[3:5] if type(x) is G1Point]))

    def prove(lo, part, states):
        P = len(part)
        gi, gpi, hi, cd, flat = [], [], [], [], [[] for _ in range(6)]
        for pr, k in zip(part, coeffs[lo: lo + P]):
            gi.extend(table._indices(pr[0], n)); gpi.extend(table._indices(pr[1], n)); hi.extend(table._indices([pr[2]], 1))
            cd.extend(bytes(x) if type(x) is not G1Point else next(enc) for x in pr[3:5])
            if any(len(e) != 48 for e in cd[-2:]):
                raise ValueError("C and D are G1Points or 48-byte encodings")
            flat[0].append(pr[5])
            for dst, src in zip(flat[1:5], pr[6:10]):
                dst.extend(src)
            if any(c is not None for c in coeffs[lo: lo + P]):
                flat[5].extend(k if k is not None else [1] * n)
        bufs = [_pack32(vals) for vals in flat]
        return table._ctx.ipa_prove_device(table._tab, n, P, gi, gpi, hi, bufs[5] if flat[5] else None, b"".join(cd), bufs[0], bufs[1], bufs[2], bufs[3],
                                           bufs[4], states)

    return _chain_prove(table, provers, transcripts, n, N.IPA_MAX_PROVERS, "the device chain of the inner-product argument runs over a FixedBaseTable",
                        prove, 2, 4, 2)


def ipa_prove_device(table, crs_G_vec, crs_G_prime_vec, crs_H, C, D, z: Scalar, vec_c: Sequence[Scalar], vec_d: Sequence[Scalar],
                     vec_r_c: Sequence[Scalar], vec_r_d: Sequence[Scalar], transcript, G_prime_coeffs: Sequence[Scalar] = None):
    """IPA.new (ipa.py:75-153) after `generate_ipa_blinders`, on the device: see ipa_prove_device_many.  `transcript` is advanced as the
    reference advances it.  -> (B_c, B_d, vec_L_C, vec_R_C, vec_L_D, vec_R_D, c_final, d_final)."""
    pr = (crs_G_vec, crs_G_prime_vec, crs_H, C, D, z, vec_c, vec_d, vec_r_c, vec_r_d) + ((G_prime_coeffs,) if G_prime_coeffs is not None else ())
    return ipa_prove_device_many(table, [pr], [transcript])[0]


def same_msm_rounds_many(provers: Sequence[Tuple[Sequence[G1Point], Sequence[G1Point], Sequence[G1Point], Sequence[Scalar]]],
                         next_gammas: Sequence[Callable[..., Scalar]]):
    """same_msm.py:93-130 for several independent provers in step: per round ONE batched MSM call (6 MSMs per prover), the
    challenges folded into the scalars as in ipa_rounds_many (the three base vectors of a prover share one coefficient vector: all
    three fold with gamma, same_msm.py:122-126).  provers[p] = (crs_G_vec, vec_T, vec_U, vec_x) with vec_x already blinded (:89-91).
    -> per prover (vec_L_A, vec_L_T, vec_L_U, vec_R_A, vec_R_T, vec_R_U, x_final)."""
    st = [dict(G=list(G), T=list(T), U=list(U), x=[v._v for v in x], out=[[] for _ in range(6)]) for G, T, U, x in provers]
    n0 = n = len(st[0]["x"])
    assert all(len(s["x"]) == len(s["G"]) == len(s["T"]) == len(s["U"]) == n for s in st) and n & (n - 1) == 0
    for s in st:
        s["k"] = [1] * n0
    R = CURVE_ORDER
    S = Scalar._raw
    while n > 1:
        n //= 2
        left, right = _halves(n0, n)
        jobs = []
        for s in st:
            x, k = s["x"], s["k"]
            sc_l = [S(x[j % (2 * n) - n] * k[j] % R) for j in right]     # x_L against the right halves
            sc_r = [S(x[n + j % (2 * n)] * k[j] % R) for j in left]      # x_R against the left halves
            for V in (s["G"], s["T"], s["U"]):                            # L_A L_T L_U
                jobs.append(([V[j] for j in right], sc_l))
            for V in (s["G"], s["T"], s["U"]):                            # R_A R_T R_U
                jobs.append(([V[j] for j in left], sc_r))
        res = compute_MSM_batch(jobs)
        for i, (s, ng) in enumerate(zip(st, next_gammas)):
            rnd = res[6 * i: 6 * i + 6]
            for lst, pnt in zip(s["out"], rnd):
                lst.append(pnt)
            gamma = ng(*rnd)._v
            gamma_inv = pow(gamma, -1, R)
            x, k = s["x"], s["k"]
            s["x"] = [(x[i] + gamma_inv * x[n + i]) % R for i in range(n)]
            for j in right:
                k[j] = k[j] * gamma % R
    return [(*s["out"], S(s["x"][0])) for s in st]


def same_msm_rounds(crs_G_vec: Sequence[G1Point], vec_T: Sequence[G1Point], vec_U: Sequence[G1Point], vec_x: Sequence[Scalar],
                    next_gamma: Callable[[G1Point, G1Point, G1Point, G1Point, G1Point, G1Point], Scalar]):
    """same_msm.py:93-130 (vec_x already blinded, :89-91).  -> (vec_L_A, vec_L_T, vec_L_U, vec_R_A, vec_R_T, vec_R_U, x_final)."""
    return same_msm_rounds_many([(crs_G_vec, vec_T, vec_U, vec_x)], [next_gamma])[0]


def same_msm_prove_device_many(table, provers: Sequence[tuple], transcripts: Sequence) -> List[tuple]:
    """SameMSMProof.new (same_msm.py:50-143) after its `generate_blinders(n)` draw, for SEVERAL independent provers of one length in step,
    proved ON THE DEVICE: one launch chain (csrc/kernels_same_msm.h), one wait.  crs_G_vec comes from the resident `table` (a
    fixed_base.FixedBaseTable); vec_T and vec_U are per-proof points, over which the call builds one light table on the device.
    provers[p] = (crs_G_vec, A, Z_t, Z_u, vec_T, vec_U, vec_x, vec_r): crs_G_vec as objects of the table or indices into it (KeyError /
    IndexError); A, Z_t, Z_u are G1Points or their 48-byte encodings (only hashed); vec_T / vec_U are G1Points (deferred ones are
    materialised in one batch; any curve point, the identity included); vec_x UNBLINDED and not mutated (the call blinds a copy with the
    alpha it draws), vec_r the caller's own blinders.
    transcripts[p]: that prover's CurdleproofsTranscript, advanced to the state after the last same_msm_gamma.
    -> per prover (B_a, B_t, B_u, vec_L_A, vec_L_T, vec_L_U, vec_R_A, vec_R_T, vec_R_U, x_final), the fields of SameMSMProof.
    A refused call (ValueError: n not a power of two >= 2; NativeError: a scalar >= r, an undecodable A, Z_t or Z_u) changes nothing."""
    from . import _native as N
    from .py_arkworks_bls12381 import points_to_affine96, points_to_compressed

    provers, n = _chain_provers(provers, transcripts, 6, "a same-MSM", N.SAME_MSM_MAX_N)
    if not provers:
        return []
    if any(not (len(pr[0]) == len(pr[4]) == len(pr[5]) == len(pr[6]) == len(pr[7]) == n) for pr in provers):
        raise ValueError("provers in step share one vector length")
    if any(type(x) is not G1Point for pr in provers for x in list(pr[4]) + list(pr[5])):
        raise TypeError("vec_T and vec_U are G1Points")
    enc = iter(points_to_compressed([x for pr in provers for x in pr[1:4] if type(x) is G1Point]))

    def prove(lo, part, states):
        gi, azz, tu, xs, rs = [], [], [], [], []
        for pr in part:
            gi.extend(table._indices(pr[0], n))
            azz.extend(bytes(x) if type(x) is not G1Point else next(enc) for x in pr[1:4])
            if any(len(e) != 48 for e in azz[-3:]):
                raise ValueError("A, Z_t and Z_u are G1Points or 48-byte encodings")
            tu.extend(pr[4]); tu.extend(pr[5])
            xs.extend(pr[6]); rs.extend(pr[7])
        return table._ctx.same_msm_prove_device(table._tab, n, len(part), gi, b"".join(azz), bytes(points_to_affine96(tu)), _pack32(xs), _pack32(rs), states)

    return _chain_prove(table, provers, transcripts, n, min(N.SAME_MSM_MAX_PROVERS, N.LIGHT_MAX_BASES // (2 * n)),
                        "the device chain of the same-MSM argument takes crs_G_vec from a FixedBaseTable", prove, 3, 6, 1)


def same_msm_prove_device(table, crs_G_vec, A, Z_t, Z_u, vec_T: Sequence[G1Point], vec_U: Sequence[G1Point], vec_x: Sequence[Scalar],
                          vec_r: Sequence[Scalar], transcript):
    """SameMSMProof.new (same_msm.py:50-143) after `vec_r = generate_blinders(n)`, on the device: see same_msm_prove_device_many.
    `transcript` is advanced as the reference advances it; vec_x is not mutated.
    -> (B_a, B_t, B_u, vec_L_A, vec_L_T, vec_L_U, vec_R_A, vec_R_T, vec_R_U, x_final)."""
    return same_msm_prove_device_many(table, [(crs_G_vec, A, Z_t, Z_u, vec_T, vec_U, vec_x, vec_r)], [transcript])[0]


def shuffle_permute_and_commit_input(crs, vec_R: Sequence[G1Point], vec_S: Sequence[G1Point], permutation: Sequence[int], k: Scalar,
                                     table=None) -> Tuple[List[G1Point], List[G1Point], G1Point, List[Scalar]]:
    """Drop-in for curdleproofs.py:301-321: vec_T = perm([R * k]), vec_U = perm([S * k]) as one same-scalar launch, M as one GPU
    MSM over vec_G | vec_H.  Draws the N_BLINDERS blinders exactly where the reference does (util.py:81-82).
    table (optional): a FixedBaseTable holding crs.vec_G and crs.vec_H (FixedBaseTable.for_crs(crs)); M then comes from the table."""
    ell = len(crs.vec_G)
    both = batch_mul_same_scalar(list(vec_R) + list(vec_S), k)
    vec_T = [both[j] for j in permutation]                               # get_permutation, util.py:93-96
    vec_U = [both[len(vec_R) + j] for j in permutation]
    sigma_ell = [Scalar(j) for j in permutation]
    vec_m_blinders = [random_scalar() for _ in range(N_BLINDERS)]
    if table is None:
        M = compute_MSM(list(crs.vec_G) + list(crs.vec_H), sigma_ell + vec_m_blinders)
    else:
        M = table.msm(sigma_ell + vec_m_blinders, list(crs.vec_G) + list(crs.vec_H))
    assert len(sigma_ell) == ell
    return vec_T, vec_U, M, vec_m_blinders


def grand_product_coeffs(ell: int, n_blinders: int, beta_inv: Scalar) -> List[Scalar]:
    """The scalars of grand_prod.py:64-71 -- beta^-(i+1) for the ell G's, beta^-(ell+1) for the blinders -- for callers that hand the base
    change to ipa_rounds as `G_prime_coeffs` instead of materialising G' / H' (grand_product_bases below: one 2.4 ms launch)."""
    out, p = [], beta_inv
    for _ in range(ell):
        out.append(p)
        p = p * beta_inv
    return out + [p] * n_blinders


def grand_product_bases(crs_G_vec: Sequence[G1Point], crs_H_vec: Sequence[G1Point], beta_inv: Scalar) -> Tuple[List[G1Point], List[G1Point]]:
    """grand_prod.py:64-71: G'_i = G_i * beta^-(i+1), H'_i = H_i * beta^-(ell+1), one per-index launch."""
    ell = len(crs_G_vec)
    pows, p = [], beta_inv
    for _ in range(ell):
        pows.append(p)
        p = p * beta_inv
    res = batch_mul(list(crs_G_vec) + list(crs_H_vec), pows + [p] * len(crs_H_vec))
    return res[:ell], res[ell:]


def grand_product_prove_device_many(table, provers: Sequence[tuple], transcripts: Sequence) -> List[tuple]:
    """GrandProductProof.new (grand_prod.py:29-119) after its random draws, for SEVERAL independent provers of one shape in step, proved ON
    THE DEVICE: one launch chain (csrc/kernels_gprod.h, then the inner-product argument's phases of csrc/kernels_ipa.h), one wait -- the
    prefix products, both gprod transcript steps, the powers of beta, the completion of the IPA's blinders, the MSMs over the resident
    `table` (a fixed_base.FixedBaseTable) and the whole inner-product argument never come back to the host.
    provers[p] = (crs_G_vec, crs_H_vec, crs_U, B, gprod_result, vec_b, vec_b_blinders, vec_c_blinders, ipa_r, ipa_z_head): bases are
    objects of the table or indices into it (KeyError / IndexError, FixedBaseTable._indices); B is a G1Point or its 48-byte encoding;
    the draws are the caller's, in the reference's order: vec_c_blinders (n_blinders), then ipa_r (n = ell + n_blinders) and ipa_z_head
    (n - 2), the two draws of generate_ipa_blinders (ipa.py:30-31) -- the device completes z.  No input is mutated.
    transcripts[p]: that prover's CurdleproofsTranscript, advanced to the state after the last ipa_gamma.
    -> per prover (C, r_p, (B_c, B_d, vec_L_C, vec_R_C, vec_L_D, vec_R_D, c_final, d_final)), the fields of GrandProductProof.
    A refused call changes nothing.  ValueError: a shape (ell >= 1, n_blinders >= 2, n a power of two).  NativeError: a scalar >= r, an
    undecodable B, and what the reference answers with an AssertionError or a division by zero -- B is not the commitment to vec_b |
    vec_b_blinders, gprod_result is not the product of vec_b, vec_c_blinders[-2] = 0, or the second denominator of generate_ipa_blinders
    is zero (draw ipa_r again)."""
    from . import _native as N
    from .py_arkworks_bls12381 import points_to_compressed

    provers, n = _chain_provers(provers, transcripts, 8, "a grand-product", N.IPA_MAX_N)
    if not provers:
        return []
    ell, nb = len(provers[0][0]), len(provers[0][1])
    if ell < 1 or nb < 2 or ell + nb != n:
        raise ValueError("a grand-product argument has ell >= 1 bases crs_G_vec, n_blinders >= 2 bases crs_H_vec and ipa_r of length ell + n_blinders")
    if any(not (len(pr[0]) == len(pr[5]) == ell and len(pr[1]) == len(pr[6]) == len(pr[7]) == nb and len(pr[8]) == n and len(pr[9]) == n - 2) for pr in provers):
        raise ValueError("provers in step share one shape (ell, n_blinders); ipa_r has n entries and ipa_z_head n - 2")
    enc = iter(points_to_compressed([pr[3] for pr in provers if type(pr[3]) is G1Point]))

    def prove(lo, part, states):
        gi, ui, b48, flat = [], [], [], [[] for _ in range(5)]
        for pr in part:
            gi.extend(table._indices(pr[0], ell)); gi.extend(table._indices(pr[1], nb)); ui.extend(table._indices([pr[2]], 1))
            b48.append(bytes(pr[3]) if type(pr[3]) is not G1Point else next(enc))
            if len(b48[-1]) != 48:
                raise ValueError("B is a G1Point or a 48-byte encoding")
            flat[0].append(pr[4])
            flat[1].extend(pr[5]); flat[1].extend(pr[6])
            for dst, src in zip(flat[2:], pr[7:10]):
                dst.extend(src)
        bufs = [_pack32(vals) for vals in flat]
        proofs, new_states = table._ctx.gprod_prove_device(table._tab, ell, nb, len(part), gi, ui, b"".join(b48), *bufs, states)
        pb = len(proofs) // len(part)
        # C | r_p | the IPA's proof  ->  points first, scalars last: what _chain_prove cuts
        cut = [proofs[pb * i: pb * i + pb] for i in range(len(part))]
        return b"".join(raw[:48] + raw[80: pb - 64] + raw[48:80] + raw[pb - 64:] for raw in cut), new_states

    res = _chain_prove(table, provers, transcripts, n, N.IPA_MAX_PROVERS, "the device chain of the grand-product argument runs over a FixedBaseTable",
                       prove, 3, 4, 3)
    return [(C, r_p, (*ipa_points, c_final, d_final)) for C, *ipa_points, r_p, c_final, d_final in res]


def grand_product_prove_device(table, crs_G_vec, crs_H_vec, crs_U, B, gprod_result: Scalar, vec_b: Sequence[Scalar], vec_b_blinders: Sequence[Scalar],
                               vec_c_blinders: Sequence[Scalar], ipa_r: Sequence[Scalar], ipa_z_head: Sequence[Scalar], transcript):
    """GrandProductProof.new (grand_prod.py:29-119) after its draws, on the device: see grand_product_prove_device_many.  `transcript` is
    advanced as the reference advances it.  -> (C, r_p, (B_c, B_d, vec_L_C, vec_R_C, vec_L_D, vec_R_D, c_final, d_final))."""
    return grand_product_prove_device_many(table, [(crs_G_vec, crs_H_vec, crs_U, B, gprod_result, vec_b, vec_b_blinders, vec_c_blinders, ipa_r, ipa_z_head)],
                                           [transcript])[0]


def same_permutation_prove_device_many(table, provers: Sequence[tuple], transcripts: Sequence) -> List[tuple]:
    """SamePermutationProof.new (same_perm.py:27-72) after its callee's random draws, for SEVERAL independent provers of one shape in step,
    proved ON THE DEVICE: the grand-product launch chain with another head (csrc/kernels_same_perm.h, then csrc/kernels_gprod.h and the
    inner-product argument's phases of csrc/kernels_ipa.h), one wait.  same_perm_step1 and the challenges same_perm_alpha / same_perm_beta
    run on the host inside the native call (they depend on nothing the device computes); the polynomial factors, their product, B and
    everything GrandProductProof.new does never come back to the host.
    provers[p] = (crs_G_vec, crs_H_vec, crs_U, A, M, vec_a, permutation, vec_a_blinders, vec_m_blinders, vec_c_blinders, ipa_r, ipa_z_head):
    bases are objects of the table or indices into it (KeyError / IndexError, FixedBaseTable._indices); A and M are G1Points or their
    48-byte encodings; permutation holds ell ints (not required to be a bijection: the reference does not require it either); the draws
    are the caller's, in the reference's order, as in grand_product_prove_device_many.  No input is mutated.
    transcripts[p]: that prover's CurdleproofsTranscript, advanced to the state after the last ipa_gamma.
    -> per prover (B, (C, r_p, (B_c, B_d, vec_L_C, vec_R_C, vec_L_D, vec_R_D, c_final, d_final))), the fields of SamePermutationProof.
    A refused call changes nothing.  ValueError: a shape (ell >= 1, n_blinders >= 2, n a power of two; a permutation entry that is not an
    int in 0 .. 2^32 - 1).  NativeError: a scalar >= r, an undecodable A or M, a permutation entry >= ell, and what the reference answers
    with an AssertionError or a division by zero -- A is not the commitment to vec_a o permutation | vec_a_blinders, M is not the
    commitment to permutation | vec_m_blinders, vec_c_blinders[-2] = 0, or the second denominator of generate_ipa_blinders is zero."""
    from . import _native as N
    from .py_arkworks_bls12381 import points_to_compressed

    provers, n = _chain_provers(provers, transcripts, 10, "a same-permutation", N.IPA_MAX_N)
    if not provers:
        return []
    ell, nb = len(provers[0][0]), len(provers[0][1])
    if ell < 1 or nb < 2 or ell + nb != n:
        raise ValueError("a same-permutation argument has ell >= 1 bases crs_G_vec, n_blinders >= 2 bases crs_H_vec and ipa_r of length ell + n_blinders")
    if any(not (len(pr[0]) == len(pr[5]) == len(pr[6]) == ell and len(pr[1]) == len(pr[7]) == len(pr[8]) == len(pr[9]) == nb and len(pr[10]) == n
                and len(pr[11]) == n - 2) for pr in provers):
        raise ValueError("provers in step share one shape (ell, n_blinders); vec_a and the permutation have ell entries, ipa_r n and ipa_z_head n - 2")
    if any(not isinstance(m, int) or not 0 <= m < 1 << 32 for pr in provers for m in pr[6]):
        raise ValueError("a permutation holds ints in 0 .. 2^32 - 1")
    enc = iter(points_to_compressed([x for pr in provers for x in pr[3:5] if type(x) is G1Point]))

    def prove(lo, part, states):
        gi, ui, am, perm, flat = [], [], [], [], [[] for _ in range(6)]
        for pr in part:
            gi.extend(table._indices(pr[0], ell)); gi.extend(table._indices(pr[1], nb)); ui.extend(table._indices([pr[2]], 1))
            am.extend(bytes(x) if type(x) is not G1Point else next(enc) for x in pr[3:5])
            if any(len(e) != 48 for e in am[-2:]):
                raise ValueError("A and M are G1Points or 48-byte encodings")
            perm.extend(pr[6])
            for dst, src in zip(flat, (pr[5],) + pr[7:12]):
                dst.extend(src)
        bufs = [_pack32(vals) for vals in flat]
        proofs, new_states = table._ctx.same_perm_prove_device(table._tab, ell, nb, len(part), gi, ui, b"".join(am), bufs[0], perm, *bufs[1:], states)
        pb = len(proofs) // len(part)
        # B | C | r_p | the IPA's proof  ->  points first, scalars last: what _chain_prove cuts
        cut = [proofs[pb * i: pb * i + pb] for i in range(len(part))]
        return b"".join(raw[:96] + raw[128: pb - 64] + raw[96:128] + raw[pb - 64:] for raw in cut), new_states

    res = _chain_prove(table, provers, transcripts, n, N.IPA_MAX_PROVERS, "the device chain of the same-permutation argument runs over a FixedBaseTable",
                       prove, 4, 4, 3)
    return [(B, (C, r_p, (*ipa_points, c_final, d_final))) for B, C, *ipa_points, r_p, c_final, d_final in res]


def same_permutation_prove_device(table, crs_G_vec, crs_H_vec, crs_U, A, M, vec_a: Sequence[Scalar], permutation: Sequence[int],
                                  vec_a_blinders: Sequence[Scalar], vec_m_blinders: Sequence[Scalar], vec_c_blinders: Sequence[Scalar], ipa_r: Sequence[Scalar],
                                  ipa_z_head: Sequence[Scalar], transcript):
    """SamePermutationProof.new (same_perm.py:27-72) after its callee's draws, on the device: see same_permutation_prove_device_many.
    `transcript` is advanced as the reference advances it.
    -> (B, (C, r_p, (B_c, B_d, vec_L_C, vec_R_C, vec_L_D, vec_R_D, c_final, d_final)))."""
    return same_permutation_prove_device_many(table, [(crs_G_vec, crs_H_vec, crs_U, A, M, vec_a, permutation, vec_a_blinders, vec_m_blinders, vec_c_blinders,
                                                       ipa_r, ipa_z_head)], [transcript])[0]


def same_scalar_prove_device_many(table, provers: Sequence[tuple], transcripts: Sequence) -> List[tuple]:
    """What CurdleProofsProof.new runs between SamePermutationProof.new and SameMSMProof.new (curdleproofs.py:92-116), for SEVERAL
    independent provers of one ell in step, proved ON THE DEVICE: R = MSM(vec_R, vec_a), S = MSM(vec_S, vec_a), cm_T, cm_U and all of
    SameScalarProof.new (same_scalar.py:39-69) as one launch chain (csrc/kernels_same_scalar.h), one wait.  R k, S k, R r_k and S r_k are
    never formed: the factors fold into the scalars, and every point the block emits is one MSM over a light table of crs_G_t | crs_G_u |
    crs_H | vec_R | vec_S the call builds on the device.  `table` (a fixed_base.FixedBaseTable) is the chain's home -- its staging block,
    its light-table scratch, its context's lock; the three CRS points need not be among its bases.
    provers[p] = (crs_G_t, crs_G_u, crs_H, vec_R, vec_S, vec_a, k, r_t, r_u, r_a, r_b, r_k): G1Points (deferred ones are materialised in
    one batch; the identity included), Scalars; the draws are the caller's, in the reference's order (r_t, r_u before the block, then r_a,
    r_b, r_k).  Provers that follow one another with the same three CRS points share a call.  No input is mutated.
    The folding is exact only for vec_R / vec_S in the prime-order subgroup: where every one of a call's entries already carries a
    membership certificate the call says so, otherwise the chain tests them on the device -- no host test is run here.
    transcripts[p]: that prover's CurdleproofsTranscript, advanced to the state after same_scalar_alpha.
    -> per prover (R, S, cm_T, cm_U, cm_A, cm_B, z_k, z_t, z_u), a commitment as the pair (T_1, T_2).
    A refused call changes nothing.  ValueError: a shape (ell in 1 .. 1024, one ell for all).  NativeError: a scalar >= r, or a vec_R /
    vec_S entry outside G1 -- that caller stays on the operators, which multiply R itself."""
    from . import _native as N
    from .py_arkworks_bls12381 import points_to_affine96

    provers = [tuple(pr) for pr in provers]
    if len(provers) != len(transcripts):
        raise ValueError("one transcript per prover")
    if not provers:
        return []
    ell = len(provers[0][3])
    if not 1 <= ell <= N.SAME_SCALAR_MAX_ELL:
        raise ValueError(f"the vectors of a same-scalar block have a length in 1 .. {N.SAME_SCALAR_MAX_ELL}, not {ell}")
    if any(len(pr) != 12 or not (len(pr[3]) == len(pr[4]) == len(pr[5]) == ell) for pr in provers):
        raise ValueError("provers in step share one vector length")
    if any(type(x) is not G1Point for pr in provers for x in list(pr[:3]) + list(pr[3]) + list(pr[4])):
        raise TypeError("crs_G_t, crs_G_u, crs_H and the entries of vec_R and vec_S are G1Points")
    S, pb = N.MERLIN_STATE_BYTES, int(N.cg1_same_scalar_proof_bytes())
    step = min(N.SAME_SCALAR_MAX_PROVERS, (N.LIGHT_MAX_BASES - 3) // (2 * ell))
    out: List[tuple] = []
    with table._ctx_lock():
        if table._KIND != "fixed-base":
            raise TypeError("the device chain of the same-scalar block runs on a FixedBaseTable's staging block and light-table scratch")
        crs = bytes(points_to_affine96([x for pr in provers for x in pr[:3]]))
        lo = 0
        while lo < len(provers):
            hi = lo + 1
            while hi < len(provers) and hi - lo < step and crs[288 * hi: 288 * hi + 288] == crs[288 * lo: 288 * lo + 288]:
                hi += 1
            part, ts = provers[lo:hi], transcripts[lo:hi]
            rs = [x for pr in part for x in list(pr[3]) + list(pr[4])]
            certified = all(x._sg is True for x in rs)
            proofs, new_states = table._ctx.same_scalar_prove_device(
                table._tab, ell, len(part), crs[288 * lo: 288 * lo + 288], bytes(points_to_affine96(rs)), _pack32([a for pr in part for a in pr[5]]),
                _pack32([pr[6] for pr in part]), _pack32([r for pr in part for r in pr[7:12]]), certified, b"".join(bytes(t.strobe._st.raw[:S]) for t in ts))
            for i, t in enumerate(ts):
                ctypes.memmove(t.strobe._st, new_states[S * i: S * i + S], S)
                raw = proofs[pb * i: pb * i + pb]
                T1, T2, U1, U2, R, S_, A1, A2, B1, B2 = (G1Point.from_compressed_bytes_unchecked(raw[48 * j: 48 * j + 48]) for j in range(10))
                z_k, z_t, z_u = (Scalar.from_le_bytes(raw[480 + 32 * j: 512 + 32 * j]) for j in range(3))
                out.append((R, S_, (T1, T2), (U1, U2), (A1, A2), (B1, B2), z_k, z_t, z_u))
            lo = hi
    return out


def same_scalar_prove_device(table, crs_G_t: G1Point, crs_G_u: G1Point, crs_H: G1Point, vec_R: Sequence[G1Point], vec_S: Sequence[G1Point],
                             vec_a: Sequence[Scalar], k: Scalar, r_t: Scalar, r_u: Scalar, r_a: Scalar, r_b: Scalar, r_k: Scalar, transcript):
    """curdleproofs.py:92-116 after the draws r_t, r_u and r_a, r_b, r_k, on the device: see same_scalar_prove_device_many.  `transcript`
    is advanced as the reference advances it.  -> (R, S, cm_T, cm_U, cm_A, cm_B, z_k, z_t, z_u), a commitment as the pair (T_1, T_2)."""
    return same_scalar_prove_device_many(table, [(crs_G_t, crs_G_u, crs_H, vec_R, vec_S, vec_a, k, r_t, r_u, r_a, r_b, r_k)], [transcript])[0]


def shuffle_draws(ell: int) -> tuple:
    """The random draws of one CurdleProofsProof.new (N_BLINDERS = 4), made with the package's own randomness in the order the reference
    makes them: vec_a_blinders (2, curdleproofs.py:73); the same-permutation callee's vec_c_blinders (4), ipa_r (n) and ipa_z_head (n - 2),
    as same_permutation_prove_device takes them; r_t, r_u (:92-93); r_a, r_b, r_k (same_scalar.py:39-41); the same-MSM vec_r (n).
    -> (vec_a_blinders, vec_c_blinders, ipa_r, ipa_z_head, r_t, r_u, r_a, r_b, r_k, vec_r), what shuffle_prove_device takes as `draws`."""
    n = ell + N_BLINDERS
    draw = lambda m: [random_scalar() for _ in range(m)]
    vec_a_blinders, vec_c_blinders, ipa_r, ipa_z_head = draw(N_BLINDERS - 2), draw(N_BLINDERS), draw(n), draw(n - 2)
    r_t, r_u, r_a, r_b, r_k = draw(5)
    return (vec_a_blinders, vec_c_blinders, ipa_r, ipa_z_head, r_t, r_u, r_a, r_b, r_k, draw(n))


def shuffle_prove_device_many(table, provers: Sequence[tuple]) -> List[bytes]:
    """CurdleProofsProof.new (curdleproofs.py:63-160) for SEVERAL independent shuffles of one ell in step, proved ON THE DEVICE in one
    native call per batch (csrc/capi_shuffle.h): the `curdleproofs` transcript is created inside the call, A and A' are table MSMs, and the
    same-permutation, same-scalar and same-MSM arguments run as one pipeline with no Python between them.
    provers[p] = (crs, vec_R, vec_S, vec_T, vec_U, M, permutation, k, vec_m_blinders, draws): crs is a CurdleproofsCrs whose vec_G, vec_H, H,
    G_t and G_u are objects of `table` (FixedBaseTable.for_crs(crs)); the vectors are G1Points (deferred ones are materialised in one batch;
    the identity included); M is a G1Point or its 48-byte encoding; permutation holds ell ints (not required to be a bijection); draws as
    shuffle_draws(ell) returns them -- the caller's, in the reference's order.  ell + 4 is a power of two in 8 .. 1024.  More provers than
    one call carries, or a change of CRS points, starts another call.  No input is mutated.
    vec_R / vec_S must lie in G1: where every one of a call's entries already carries a membership certificate the call says so, otherwise
    the chain tests them on the device.
    -> per prover CurdleProofsProof.to_bytes(), byte for byte what the reference writes for those inputs and draws.
    A refused call changes nothing.  ValueError / TypeError: a shape or a type.  NativeError: a scalar >= r, a point off the curve, a
    vec_R / vec_S entry outside G1, a permutation entry >= ell, an M that is not the commitment to permutation | vec_m_blinders, and the
    divisions by zero of generate_ipa_blinders."""
    from . import _native as N
    from .py_arkworks_bls12381 import points_to_affine96, points_to_compressed

    provers = [tuple(pr) for pr in provers]
    if not provers:
        return []
    if any(len(pr) != 10 for pr in provers):
        raise ValueError("a prover is (crs, vec_R, vec_S, vec_T, vec_U, M, permutation, k, vec_m_blinders, draws)")
    ell = len(provers[0][1])
    n = ell + N_BLINDERS
    if ell < 1 or n & (n - 1) or n > N.SAME_MSM_MAX_N:
        raise ValueError(f"a shuffle proof has ell + {N_BLINDERS} a power of two in 8 .. {N.SAME_MSM_MAX_N}, not ell = {ell}")
    for pr in provers:
        crs, dr = pr[0], tuple(pr[9])
        if not (len(pr[1]) == len(pr[2]) == len(pr[3]) == len(pr[4]) == len(pr[6]) == len(crs.vec_G) == ell and len(crs.vec_H) == N_BLINDERS == len(pr[8])):
            raise ValueError("provers in step share one ell; the four vectors, the permutation and crs.vec_G have ell entries, crs.vec_H and vec_m_blinders 4")
        if len(dr) != 10 or not (len(dr[0]) == 2 and len(dr[1]) == N_BLINDERS and len(dr[2]) == n and len(dr[3]) == n - 2 and len(dr[9]) == n):
            raise ValueError("draws are (vec_a_blinders (2), vec_c_blinders (4), ipa_r (n), ipa_z_head (n - 2), r_t, r_u, r_a, r_b, r_k, vec_r (n))")
        if any(not isinstance(m, int) or not 0 <= m < 1 << 32 for m in pr[6]):
            raise ValueError("a permutation holds ints in 0 .. 2^32 - 1")
        if any(type(x) is not G1Point for v in pr[1:5] for x in v) or any(type(x) is not G1Point for x in (crs.H, crs.G_t, crs.G_u)):
            raise TypeError("crs.G_t, crs.G_u, crs.H and the entries of vec_R, vec_S, vec_T and vec_U are G1Points")
        if any(type(x) is not Scalar for x in [pr[7], *pr[8], *dr[0], *dr[1], *dr[2], *dr[3], *dr[4:9], *dr[9]]):
            raise TypeError("k, vec_m_blinders and the draws are Scalars")
    enc = iter(points_to_compressed([pr[5] for pr in provers if type(pr[5]) is G1Point]))
    m48 = [bytes(pr[5]) if type(pr[5]) is not G1Point else next(enc) for pr in provers]
    if any(len(e) != 48 for e in m48):
        raise ValueError("M is a G1Point or a 48-byte encoding")
    pb = int(N.cg1_shuffle_prover_proof_bytes(ell))
    step = min(N.SAME_MSM_MAX_PROVERS, N.LIGHT_MAX_BASES // (2 * n))
    out: List[bytes] = []
    with table._ctx_lock():
        if table._KIND != "fixed-base":
            raise TypeError("the device pipeline of a shuffle proof runs over a FixedBaseTable")
        gth = bytes(points_to_affine96([x for pr in provers for x in (pr[0].G_t, pr[0].G_u, pr[0].H)]))
        lo = 0
        while lo < len(provers):
            hi = lo + 1
            while hi < len(provers) and hi - lo < step and gth[288 * hi: 288 * hi + 288] == gth[288 * lo: 288 * lo + 288]:
                hi += 1
            part = provers[lo:hi]
            gi, hi_, ui, gti, gui, perm = [], [], [], [], [], []
            for pr in part:
                crs = pr[0]
                gi.extend(table._indices(crs.vec_G, ell)); hi_.extend(table._indices(crs.vec_H, N_BLINDERS))
                ui.extend(table._indices([crs.H], 1)); gti.extend(table._indices([crs.G_t], 1)); gui.extend(table._indices([crs.G_u], 1))
                perm.extend(pr[6])
            rs = [x for pr in part for x in list(pr[1]) + list(pr[2])]
            tu = [x for pr in part for x in list(pr[3]) + list(pr[4])]
            certified = all(x._sg is True for x in rs)
            dr = [tuple(pr[9]) for pr in part]
            proofs = table._ctx.shuffle_prove_device(
                table._tab, ell, len(part), gi, hi_, ui, gti, gui, gth[288 * lo: 288 * lo + 288], bytes(points_to_affine96(rs)), bytes(points_to_affine96(tu)),
                b"".join(m48[lo:hi]), perm, _pack32([pr[7] for pr in part]), _pack32([b for pr in part for b in pr[8]]), _pack32([b for d in dr for b in d[0]]),
                _pack32([b for d in dr for b in d[1]]), _pack32([b for d in dr for b in d[2]]), _pack32([b for d in dr for b in d[3]]),
                _pack32([b for d in dr for b in d[4:9]]), _pack32([b for d in dr for b in d[9]]), certified)
            out.extend(proofs[pb * i: pb * i + pb] for i in range(len(part)))
            lo = hi
    return out


def shuffle_prove_device(table, crs, vec_R: Sequence[G1Point], vec_S: Sequence[G1Point], vec_T: Sequence[G1Point], vec_U: Sequence[G1Point], M,
                         permutation: Sequence[int], k: Scalar, vec_m_blinders: Sequence[Scalar], draws: tuple) -> bytes:
    """CurdleProofsProof.new(crs, vec_R, vec_S, vec_T, vec_U, M, permutation, k, vec_m_blinders).to_bytes() with the caller's `draws`
    (shuffle_draws(ell)), on the device: see shuffle_prove_device_many."""
    return shuffle_prove_device_many(table, [(crs, vec_R, vec_S, vec_T, vec_U, M, permutation, k, vec_m_blinders, draws)])[0]
