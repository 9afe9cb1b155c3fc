"""The placement map of a seeded Whisk shuffle's witness (csrc/whisk_shuffle_host.h: PLACE_RULES, place_source), which the device kernel
k_whisk_witness_place and the host emulation share, held against the copying path's own staging code -- ShuffleWitness::gather and the
*_stage functions -- through cg1_whisk_witness_block_emulate.  No GPU.

The draws' block is filled with the 32-bit counters 1, 2, 3, ..: every word of a staged block then names the word of the draws it came
from, and 0 is a byte nothing was copied into.  Per shape and keep list: the block staged by the copying path (resident = 0) and the block
placed by the map (resident = 1) are the same bytes over the whole block, the front's and the chain's; nothing outside the listed witness
fields is written; and the words the fields hold are exactly the rows the column table gives the provers in question -- the permutations
and every column, each row at its column_width, no word of a dropped prover, of the Fisher-Yates swaps or of the padding."""
import ctypes

import numpy as np
import pytest

NB = 4
SYMBOLS = ["cg1_whisk_last_witness_traffic", "cg1_whisk_draws_buffer_is_zero", "cg1_whisk_witness_block_emulate"]
FRONT, CHAIN = 0, 1
COLUMNS = ("k", "vec_m_blinders", "vec_a_blinders", "vec_c_blinders", "ipa_r", "ipa_z_head", "blinders", "vec_r")


def column_width(ell):
    n = ell + NB
    return dict(zip(COLUMNS, (1, NB, 2, NB, n, n - 2, 5, n)))


def draw_block(ell, P):
    """DrawBlock of whisk_shuffle_host.h, restated: swaps | perm | scalars, each on a 64-byte boundary -> (perm, scalars, total) in bytes"""
    up = lambda b: (b + 63) & ~63
    perm = up(P * (ell - 1) * 4)
    scalars = perm + up(P * ell * 4)
    return perm, scalars, scalars + 32 * P * sum(column_width(ell).values())


def rows(ell, P, provers, columns):
    """the words (numbered from 1, as the counters are) of the draws' block that hold the permutation rows of `provers` and their rows of `columns`"""
    perm, scalars, _ = draw_block(ell, P)
    want = [np.arange(perm // 4 + p * ell, perm // 4 + (p + 1) * ell) for p in provers]
    at = scalars // 4
    for name, w in column_width(ell).items():
        if name in columns:
            want += [np.arange(at + 8 * w * p, at + 8 * w * (p + 1)) for p in provers]
        at += 8 * w * P
    return np.unique(np.concatenate(want)) + 1


def emulate(N, ell, P, keep, draws, resident, block):
    arr = (ctypes.c_size_t * len(keep))(*keep)
    nf = ctypes.c_size_t(0)
    total = N.cg1_whisk_witness_block_emulate(ell, P, arr, len(keep), draws, resident, block, None, 0, None, ctypes.byref(nf))
    assert total > 0 and nf.value > 0, (ell, P, keep, block)
    out = ctypes.create_string_buffer(b"\xaa" * total, total)
    fields = (ctypes.c_uint64 * (2 * nf.value))()
    again = ctypes.c_size_t(nf.value)
    assert N.cg1_whisk_witness_block_emulate(ell, P, arr, len(keep), draws, resident, block, out, total, fields, ctypes.byref(again)) == total
    assert again.value == nf.value
    return out.raw, [(int(fields[2 * i]), int(fields[2 * i + 1])) for i in range(nf.value)]


def keep_lists(P):
    every = list(range(P))
    lists = [every, every[1:], every[: P // 2] + every[P // 2 + 1:], every[:-1], every[-1:]]
    out = []
    for k in lists:
        if k and k not in out:
            out.append(k)
    return out


def test_symbols_and_header(native_lib):
    import os

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "curdle_g1.h")).read()
    for name in SYMBOLS:
        assert hasattr(native_lib.lib, name) and name + "(" in header, name
    assert '"whisk_resident_witness"' in header


@pytest.mark.parametrize("ell", [4, 12, 60, 124])
@pytest.mark.parametrize("P", [1, 3, 5, 64])
def test_the_map_places_what_the_copying_path_stages(native_lib, ell, P):
    N = native_lib
    n = ell + NB
    assert P * 2 * n <= N.LIGHT_MAX_BASES
    perm_at, scalars_at, total = draw_block(ell, P)
    draws = np.arange(1, total // 4 + 1, dtype="<u4").tobytes()
    assert len(draws) == total
    for keep in keep_lists(P):
        for block in (FRONT, CHAIN):
            staged, fields = emulate(N, ell, P, keep, draws, 0, block)
            placed, fields1 = emulate(N, ell, P, keep, draws, 1, block)
            assert fields == fields1
            assert staged == placed, (ell, P, keep, block)
            # ---- nothing outside the listed fields, and the fields do not overlap
            mask = np.zeros(len(placed), dtype=bool)
            for off, length in fields:
                assert length > 0 and off % 64 == 0 and off + length <= len(placed) and not mask[off: off + length].any(), (off, length)
                mask[off: off + length] = True
            got = np.frombuffer(placed, dtype=np.uint8)
            assert not got[~mask].any(), (ell, P, keep, block)
            # ---- the fields hold exactly the rows of the column table: the front's block every prover's permutation, k and vec_m_blinders;
            # the chain's block the kept provers' permutations and all eight columns, each row at its full width
            words = np.concatenate([np.frombuffer(placed[off: off + length], dtype="<u4") for off, length in fields])
            used = np.unique(words[words != 0])
            want = rows(ell, P, range(P), ("k", "vec_m_blinders")) if block == FRONT else rows(ell, P, keep, COLUMNS)
            assert np.array_equal(used, want), (ell, P, keep, block)
            # ---- and the destination prover q reads source prover keep[q]: the first word of every field's q-th row
            provers = list(range(P)) if block == FRONT else keep
            for off, length in fields:
                row = length // len(provers)
                assert row * len(provers) == length
                first = np.frombuffer(placed, dtype="<u4", count=1, offset=off)[0], np.frombuffer(placed, dtype="<u4", count=1, offset=off + row * (len(provers) - 1))[0]
                for word, p in zip(first, (provers[0], provers[-1])):
                    src = 4 * (int(word) - 1)
                    if src < scalars_at:
                        assert perm_at + 4 * ell * p <= src < perm_at + 4 * ell * (p + 1), (off, p)
                    else:
                        assert src in {scalars_at + 32 * (P * sum(list(column_width(ell).values())[:c]) + w * p) for c, w in enumerate(column_width(ell).values())}, (off, p)


def test_the_emulation_refuses_what_the_entry_would_not_reach(native_lib):
    N = native_lib
    nf = ctypes.c_size_t(0)
    draws = bytes(draw_block(4, 3)[2])
    call = lambda ell, P, keep, block: N.cg1_whisk_witness_block_emulate(ell, P, (ctypes.c_size_t * max(1, len(keep)))(*keep), len(keep), draws, 1, block, None, 0, None,
                                                                         ctypes.byref(nf))
    assert call(4, 3, [0, 1, 2], CHAIN) > 0
    for ell, P, keep, block in ((5, 3, [0], CHAIN), (4, 0, [0], CHAIN), (4, 65, [0], CHAIN), (4, 3, [3], CHAIN), (4, 3, [1, 1], CHAIN), (4, 3, [2, 1], CHAIN), (4, 3, [0], 2)):
        assert call(ell, P, keep, block) == 0, (ell, P, keep, block)
    # a buffer too small for the block is not written
    total = call(4, 3, [0, 2], CHAIN)
    out = ctypes.create_string_buffer(b"\xaa" * total, total)
    keep = (ctypes.c_size_t * 2)(0, 2)
    assert N.cg1_whisk_witness_block_emulate(4, 3, keep, 2, draws, 1, CHAIN, out, total - 1, None, ctypes.byref(nf)) == total and out.raw == b"\xaa" * total
