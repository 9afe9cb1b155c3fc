"""What a seed draws for a Whisk shuffle, without a GPU: shuffle_prover.shuffle_draws_from_seed against the
derivation written out with hashlib (tests/whisk_shuffle_seeded_cases.py) and against the committed golden file, the host twin
cg1_whisk_shuffle_draws against the same model, the refusals of the draw entries, and the length checks of the Python face."""
import ctypes
import json
import os
import types

import pytest

import whisk_shuffle_seeded_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, NB = S.R, S.NB


@pytest.mark.parametrize("ell", (4, 12, 124))
def test_the_python_model_is_the_written_out_derivation(native_lib, ell):
    from curdleproofs_pie_amd.shuffle_prover import shuffle_draws_from_seed

    for seed, index in ((S.SEED_A, 0), (S.SEED_B, 7), (S.SEED_B, (1 << 32) - 1)):
        perm, scalars = S.model(seed, index, ell)
        got = shuffle_draws_from_seed(seed, index, ell)
        assert got == S.as_item(perm, scalars, ell), (ell, index)
        assert sorted(got[0]) == list(range(ell))                        # a bijection
        assert len(scalars) == 3 * (ell + NB) + 14 and all(0 <= v < R for v in scalars)
        flat = [got[1], *got[2]] + [x for d in got[3] for x in (d if isinstance(d, list) else [d])]
        assert len(flat) == len(scalars) and all(len(b) == 32 and int.from_bytes(b, "little") < R for b in flat)
    # another seed, index or ell draws something else
    assert shuffle_draws_from_seed(S.SEED_A, 0, ell) != shuffle_draws_from_seed(S.SEED_A, 1, ell)
    assert shuffle_draws_from_seed(S.SEED_A, 0, ell)[1] != shuffle_draws_from_seed(S.SEED_B, 0, ell)[1]


def test_the_fisher_yates_steps_by_hand():
    """ell = 4 spelt out: three swaps from the first 16 bytes of blocks 0, 1, 2, the moduli 4, 3, 2."""
    perm = [0, 1, 2, 3]
    for d, i in ((0, 3), (1, 2), (2, 1)):
        j = int.from_bytes(S.block(S.SEED_A, 5, d)[:16], "little") % (i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    assert S.model(S.SEED_A, 5, 4)[0] == perm


def test_the_golden_file_fixes_the_format(native_lib):
    from curdleproofs_pie_amd.shuffle_prover import shuffle_draws_from_seed

    with open(os.path.join(ROOT, "tests", "golden", "whisk_shuffle_seeded_vectors.json")) as f:
        cases = json.load(f)["cases"]
    assert {c["ell"] for c in cases} == {4, 12}
    h = bytes.fromhex
    for c in cases:
        perm, k, mbl, draws = shuffle_draws_from_seed(h(c["seed"]), c["index"], c["ell"])
        assert perm == c["permutation"] and k == h(c["k"]) and mbl == [h(x) for x in c["vec_m_blinders"]]
        want = tuple([h(x) for x in c[key]] if isinstance(c[key], list) else h(c[key])
                     for key in ("vec_a_blinders", "vec_c_blinders", "ipa_r", "ipa_z_head", "r_t", "r_u", "r_a", "r_b", "r_k", "vec_r"))
        assert draws == want, (c["ell"], c["index"])
        # ... and the hashlib model of the tests agrees with the file's generator
        assert S.as_item(*S.model(h(c["seed"]), c["index"], c["ell"]), c["ell"]) == (perm, k, mbl, draws)


def host_draws(N, ell, count, seed, first_index, null=()):
    """cg1_whisk_shuffle_draws -> (rc, perm, scalars); the outputs are pre-filled with 0xAA."""
    ns = 3 * (ell + NB) + 14
    perm = (ctypes.c_uint32 * max(1, ell * count))(*([0xAAAAAAAA] * max(1, ell * count)))
    sc = ctypes.create_string_buffer(b"\xaa" * max(1, 32 * ns * count), max(1, 32 * ns * count))
    rc = N.cg1_whisk_shuffle_draws(ell, count, None if "seed" in null else seed, first_index, None if "perm" in null else perm, None if "scalars" in null else sc)
    return rc, list(perm), sc.raw


@pytest.mark.parametrize("ell", (4, 12, 124))
def test_the_host_twin_equals_the_model(native_lib, ell):
    for count in (1, 3, 65):
        for first in (0, 7, (1 << 32) - 65):
            rc, perm, sc = host_draws(native_lib, ell, count, S.SEED_A, first)
            want_perm, want_sc = S.columns(S.SEED_A, first, ell, count)
            assert rc == native_lib.OK and perm == want_perm and sc == want_sc, (ell, count, first)
    rc, perm, sc = host_draws(native_lib, ell, 1, S.SEED_B, 3)
    assert (perm, sc) == S.columns(S.SEED_B, 3, ell, 1)


def test_the_host_twin_refuses_and_writes_nothing(native_lib):
    N = native_lib
    untouched = lambda perm, sc: all(v == 0xAAAAAAAA for v in perm) and sc == b"\xaa" * len(sc)
    for kw in (dict(ell=5), dict(ell=0), dict(ell=2044), dict(count=N.WHISK_SHUFFLE_DRAWS_MAX_PROVERS + 1), dict(first=(1 << 32) - 2, count=3), dict(first=1 << 32, count=1),
               dict(first=(1 << 64) - 1, count=2), dict(null=("seed",)), dict(null=("perm",)), dict(null=("scalars",))):
        ell, count = kw.get("ell", 4), kw.get("count", 3)
        # (the buffers are sized for a legal shape: a refusal must not touch them whatever it was asked)
        size_ell, size_count = (ell if ell in (4, 12) else 4), min(count, 8)
        ns = 3 * (size_ell + NB) + 14
        perm = (ctypes.c_uint32 * (size_ell * size_count))(*([0xAAAAAAAA] * (size_ell * size_count)))
        sc = ctypes.create_string_buffer(b"\xaa" * (32 * ns * size_count), 32 * ns * size_count)
        null = kw.get("null", ())
        rc = N.cg1_whisk_shuffle_draws(ell, count, None if "seed" in null else S.SEED_A, kw.get("first", 0), None if "perm" in null else perm,
                                       None if "scalars" in null else sc)
        assert rc == N.ERR_ARG and untouched(list(perm), sc.raw), kw
    rc, perm, sc = host_draws(N, 4, 2, S.SEED_A, (1 << 32) - 2)              # the last two indices are legal
    assert rc == N.OK and (perm, sc) == S.columns(S.SEED_A, (1 << 32) - 2, 4, 2)
    assert N.cg1_whisk_shuffle_draws(4, 0, S.SEED_A, 1 << 32, (ctypes.c_uint32 * 1)(), ctypes.create_string_buffer(1)) == N.OK      # nothing to draw


def test_the_python_face_checks_lengths_before_anything_runs(native_lib):
    """No table, no context: a wrong length raises before either is touched."""
    from curdleproofs_pie_amd.shuffle_prover import REJECT_NAMES, ShuffleBatchProver, shuffle_draws_from_seed

    crs = types.SimpleNamespace(vec_G=[None] * 4, vec_H=[None] * 4, H=None, G_t=None, G_u=None)
    prover = ShuffleBatchProver(crs, table=object())
    with pytest.raises(ValueError, match="trackers96"):
        prover.generate_packed(bytes(96 * 4 + 1), seed=S.SEED_A)
    with pytest.raises(ValueError, match="trackers96"):
        prover.generate_packed(bytes(96 * 3), seed=S.SEED_A)
    for bad in (bytes(31), bytes(33), b""):
        with pytest.raises(ValueError, match="seed"):
            prover.generate_packed(bytes(96 * 4), seed=bad)
        with pytest.raises(ValueError, match="seed"):
            shuffle_draws_from_seed(bad, 0, 4)
    with pytest.raises(ValueError, match="first_index"):
        prover.generate_packed(bytes(96 * 4 * 2), seed=S.SEED_A, first_index=(1 << 32) - 1)
    with pytest.raises(ValueError, match="first_index"):
        prover.generate_packed(bytes(96 * 4), seed=S.SEED_A, first_index=-1)
    with pytest.raises(ValueError, match="index"):
        shuffle_draws_from_seed(S.SEED_A, 1 << 32, 4)
    with pytest.raises(ValueError, match="ell"):
        prover.generate_seeded([[(bytes(48), bytes(48))] * 3], seed=S.SEED_A)
    with pytest.raises(ValueError, match="48-byte"):
        prover.generate_seeded([[(bytes(48), bytes(47))] * 4], seed=S.SEED_A)
    assert prover.generate_packed(b"", seed=S.SEED_A) == (b"", b"", []) and prover.generate_seeded([]) == []
    assert REJECT_NAMES[0] == "proved" and set(REJECT_NAMES) == {0, 2, 3}
