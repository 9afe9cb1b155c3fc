"""The batched Whisk shuffle prover from tracker bytes, the parts that run without a GPU: cg1_whisk_shuffle_front_emulate -- the host twin
of the device front cg1_whisk_shuffle_front, with the same refusals and texts (csrc/whisk_shuffle_host.h) -- against the CPU oracle on
the fixture cases, the edge inputs and the refusals of tests/whisk_shuffle_cases.py; the wire length; the symbol lists; and the shape and
type errors of shuffle_prover.ShuffleBatchProver.prove_many, which are raised before anything native runs."""
import ctypes
import json
import os
import types

import pytest

import whisk_shuffle_cases as W

R, NB, INF = W.R, W.NB, W.INF
SYMBOLS = ["cg1_whisk_shuffle_proof_bytes", "cg1_whisk_shuffle_front", "cg1_whisk_shuffle_prove_device", "cg1_whisk_shuffle_front_emulate"]


def emulate(N, f, gh=True, raw=None, ell=None, null=()):
    """-> (rc, text, dict of the five outputs as bytes); the outputs are pre-filled with 0xAA."""
    from curdleproofs_pie_amd.py_arkworks_bls12381 import G1Point, points_to_affine96

    ell_ = f.ell if ell is None else ell
    n = f.ell + NB
    raw = dict(getattr(f, "raw", {}), **(raw or {}))
    fill = lambda m: ctypes.create_string_buffer(b"\xaa" * m, m)
    out = {"rs": fill(192 * f.ell), "tu": fill(192 * f.ell), "post": fill(96 * f.ell), "row": fill(32 * n), "m48": fill(48)}
    gh96 = bytes(points_to_affine96([G1Point.from_compressed_bytes_unchecked(e) for e in W.crs_encodings(f.ell)])) if gh else None
    args = {"trackers96": f.trackers96, "perm": (ctypes.c_uint32 * f.ell)(*f.perm), "k32": raw.get("k32", f.k32), "mbl32": raw.get("mbl32", f.mbl32), "gh": gh96, **out}
    for key in null:
        args[key] = None
    err = ctypes.create_string_buffer(256)
    rc = N.cg1_whisk_shuffle_front_emulate(ell_, args["trackers96"], args["perm"], args["k32"], args["mbl32"], args["gh"], args["rs"], args["tu"], args["post"],
                                           args["row"], args["m48"], err)
    return rc, err.value.decode(), {key: v.raw for key, v in out.items()}


def untouched(out):
    return all(v == b"\xaa" * len(v) for v in out.values())


def test_symbols_and_wire_length(native_lib):
    N = native_lib
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in N.EXPORTED_SYMBOLS, name
    for ell in (0, 3, 5, N.SAME_MSM_MAX_N - NB + 1):
        assert N.cg1_whisk_shuffle_proof_bytes(ell) == 0
    for ell in (4, 12, 28, 124, N.SAME_MSM_MAX_N - NB):
        assert N.cg1_whisk_shuffle_proof_bytes(ell) == 48 + N.cg1_shuffle_prover_proof_bytes(ell)
    for c in json.load(open(os.path.join(W.ROOT, "tests", "golden", "whisk_shuffle_prover_vectors.json")))["cases"]:
        assert [len(p) // 2 for p in c["proofs"]] == [N.cg1_whisk_shuffle_proof_bytes(c["ell"])] * 2
    assert N.cg1_whisk_shuffle_front(None, None, 4, 1, *([None] * 10)) == N.ERR_HIP                  # before a context is looked at
    assert N.cg1_whisk_shuffle_prove_device(None, None, 4, 1, *([None] * 18)) == N.ERR_HIP


@pytest.mark.parametrize("which", range(3))
def test_fixture_cases(native_lib, which):
    """ell = 4, 12, 28: vec_R / vec_S encodings in, the case's vec_T, vec_U and M encodings out, the affine records of the oracle-decoded
    points, and perm | blinders as M's scalar row."""
    f, c = W.fixture_fronts()[which]
    rc, text, out = emulate(native_lib, f)
    assert rc == native_lib.OK and text == ""
    want_post = b"".join(bytes.fromhex(t) + bytes.fromhex(u) for t, u in zip(c["vec_T"], c["vec_U"]))
    assert out["post"] == want_post and out["m48"].hex() == c["M"]
    e = f.expected
    assert e["post"] == want_post and e["m48"].hex() == c["M"]                                    # the oracle agrees with the reference's record
    assert out["rs"] == e["rs"] and out["tu"] == e["tu"] and out["row"] == e["row"]
    rc, _, out2 = emulate(native_lib, f, gh=False)                                                # without the CRS: everything but M
    assert rc == native_lib.OK and out2["m48"] == b"\xaa" * 48 and {k: v for k, v in out2.items() if k != "m48"} == {k: v for k, v in out.items() if k != "m48"}


@pytest.mark.parametrize("name", list(W.edge_fronts()))
def test_edge_inputs(native_lib, name):
    f = W.edge_fronts()[name]
    rc, text, out = emulate(native_lib, f)
    assert rc == native_lib.OK, text
    e = f.expected
    for key in ("rs", "tu", "post", "row", "m48"):
        assert out[key] == e[key], (name, key)
    post = [out["post"][48 * i: 48 * i + 48] for i in range(2 * f.ell)]
    if name == "k = 0":
        assert post == [INF] * 8 and out["tu"] == bytes(192 * f.ell)
    if name == "canonical identity":
        assert post.count(INF) == 4 and out["rs"][: 96] == bytes(96)
    if name == "lenient identities":
        assert post.count(INF) == 4
    if name in ("k = 1", "k = r - 1"):
        one = W.edge_fronts()["k = 1"]
        permuted = [one.trackers[j][h] for j in one.perm for h in (0, 1)]
        assert [p[1:] for p in post] == [q[1:] for q in permuted]
        assert all(W.sign_bit(p) == (W.sign_bit(q) != (name == "k = r - 1")) for p, q in zip(post, permuted))      # k = r - 1 negates: every sign bit flips
    if name == "no bijection":
        assert post[0:2] == post[2:4] == post[6:8] != post[4:6]
    if name == "repeated trackers":
        assert post[2:4] == post[4:6] == post[6:8] != post[0:2]                                      # trackers 0, 1 and 3 are one tracker; perm = [2, 0, 3, 1]
    if name == "both signs":
        ins = [enc for t in f.trackers for enc in t]
        assert {W.sign_bit(x) for x in ins} == {True, False} and {W.sign_bit(x) for x in post} == {True, False}


def test_refusals_leave_the_outputs_untouched(native_lib):
    N = native_lib
    base = W.edge_fronts()["both signs"]
    who = "cg1_whisk_shuffle_front_emulate"
    assert emulate(N, base)[0] == N.OK
    for name, status, edit, fragments in W.refusals():
        rc, text, out = emulate(N, edit(base))
        assert rc == getattr(N, status), (name, rc, text)
        assert untouched(out), name
        assert text.startswith(who + ": ") and "prover 0" in text, (name, text)
        for frag in fragments:
            assert frag in text, (name, text)
        if fragments:                                                                             # the half is named exactly: "r_G" is a substring of "k_r_G"
            assert ("k_r_G" in text) == (fragments[1] == "k_r_G"), (name, text)
    rc, text, out = emulate(N, base, ell=5)
    assert rc == N.ERR_ARG and untouched(out) and text.startswith(who) and "power of two" in text
    for key in ("trackers96", "perm", "k32", "mbl32", "rs", "tu", "post", "row", "m48"):
        rc, text, out = emulate(N, base, null=(key,))
        assert rc == N.ERR_ARG and untouched(out) and "bad argument" in text, key
    assert emulate(N, base)[0] == N.OK
    # the first refusal in tracker order wins, the decoder's before the subgroup test's
    two = W.refusals()[4][2](W.refusals()[0][2](base))                                            # tracker 1 r_G: no flag; tracker 2 r_G: outside G1
    rc, text, _ = emulate(N, two)
    assert rc == N.ERR_ENCODING and "tracker 1" in text


class Untouchable:
    """Stands in for a table: any use is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"the table was touched ({name}) before the arguments were checked")


def test_prove_many_checks_shapes_and_types_first(native_lib):
    from curdleproofs_pie_amd.shuffle_prover import ShuffleBatchProver

    ell, n = 4, 8
    crs = types.SimpleNamespace(vec_G=[None] * ell, vec_H=[None] * NB, H=None, G_t=None, G_u=None)
    prover = ShuffleBatchProver(crs, table=Untouchable())
    f = W.edge_fronts()["both signs"]
    draws = ([1, 2], [1, 2, 3, 4], [5] * n, [6] * (n - 2), 1, 2, 3, 4, 5, [7] * n)
    good = (f.trackers, f.perm, f.k, f.mbl, draws)
    edit = lambda i, v: good[:i] + (v,) + good[i + 1:]
    bad_value = [good[:4], edit(0, f.trackers[:-1]), edit(0, f.trackers[:-1] + [(b"\x00" * 47, f.trackers[0][1])]), edit(1, f.perm[:-1]), edit(1, f.perm[:-1] + [-1]),
                 edit(1, f.perm[:-1] + [1 << 32]), edit(2, 1 << 256), edit(2, b"\x00" * 31), edit(3, f.mbl[:-1]), edit(4, draws[:-1]),
                 edit(4, draws[:2] + ([5] * (n - 1),) + draws[3:]), edit(4, draws[:9] + ([7] * (n + 1),))]
    for item in bad_value:
        with pytest.raises(ValueError):
            prover.prove_many([good, item])
    for item in (edit(1, f.perm[:-1] + [1.5]), edit(1, f.perm[:-1] + [True]), edit(2, None), edit(0, f.trackers[:-1] + [5])):
        with pytest.raises(TypeError):
            prover.prove_many([item])
    assert prover.prove_many([]) == []
    with pytest.raises(ValueError):
        ShuffleBatchProver(types.SimpleNamespace(vec_G=[None] * 5, vec_H=[None] * NB, H=None, G_t=None, G_u=None), table=Untouchable())      # ell = 5
    with pytest.raises(ValueError):
        ShuffleBatchProver(types.SimpleNamespace(vec_G=[None] * 4, vec_H=[None] * 3, H=None, G_t=None, G_u=None), table=Untouchable())
    with pytest.raises(AssertionError, match="touched"):
        prover.prove_many([good])                                                                 # a well-formed item does reach the table
    prover.close()                                                                                # a table the prover did not make is not closed by it
