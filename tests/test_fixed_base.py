"""Fixed-base tables, the parts that run without a GPU: the signed 8-bit recoding the kernel computes (cg1_fixed_digits is compiled
from the function the kernel runs, csrc/fixed_digits.h), the three symbol lists, and the no-GPU failure mode of the Python class."""
import ctypes
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
FIXED = ["cg1_fixed_create", "cg1_fixed_destroy", "cg1_fixed_len", "cg1_fixed_bytes", "cg1_fixed_msm", "cg1_fixed_msm_device", "cg1_fixed_digits"]


def digits(N, k):
    out = (ctypes.c_int16 * 32)()
    N.cg1_fixed_digits(k.to_bytes(32, "little"), out)
    return list(out)


def check(N, k):
    d = digits(N, k)
    assert all(-128 <= v <= 128 for v in d), (hex(k), d)
    assert sum(v << (8 * w) for w, v in enumerate(d)) == k, (hex(k), d)
    return d


def test_digits_edge_scalars(native_lib):
    assert check(native_lib, 0) == [0] * 32
    assert check(native_lib, 1) == [1] + [0] * 31
    check(native_lib, R - 1)
    assert check(native_lib, 128) == [128] + [0] * 31           # 128 stays a positive digit
    assert check(native_lib, 129)[:2] == [-127, 1]              # 129 = 256 - 127


def test_digits_repeated_bytes(native_lib):
    """Every scalar made of one repeated byte 0x7f / 0x80 / 0x81 that is below r: all lengths, 32 bytes included where it fits."""
    seen = 0
    for byte in (0x7F, 0x80, 0x81):
        for length in range(1, 33):
            k = int.from_bytes(bytes([byte]) * length, "little")
            if k < R:
                check(native_lib, k)
                seen += 1
    assert seen >= 3 * 31
    assert int.from_bytes(b"\x7f" * 32, "little") >= R          # the 32-byte forms of all three lie above r: 31 bytes is the longest


def test_digits_carry_chains(native_lib):
    """Runs of 0xff bytes: the carry walks through every window of the run."""
    rng = random.Random(7)
    for start in range(0, 31):
        for length in range(1, 32 - start):
            k = int.from_bytes(b"\xff" * length, "little") << (8 * start)
            if k < R:
                d = check(native_lib, k)
                assert d[start] == -1 and d[start + length] == 1 and not any(d[start + 1: start + length])
            k2 = (k | rng.getrandbits(8 * start)) if start else k
            if k2 < R:
                check(native_lib, k2)
    check(native_lib, int.from_bytes(b"\xff" * 31 + b"\x72", "little"))      # a carry into the top window: 0x72 + 1 <= 0x73, still below r


def test_digits_random(native_lib):
    rng = random.Random(8)
    for _ in range(2000):
        check(native_lib, rng.randrange(R))


def test_symbol_lists_agree(native_lib):
    src = open(os.path.join(ROOT, "include", "curdle_g1.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cg1_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(native_lib.LIB_PATH)
    for name in FIXED:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in native_lib.EXPORTED_SYMBOLS, name
        assert callable(getattr(native_lib, name)), name
    assert sorted(native_lib.EXPORTED_SYMBOLS) == sorted(declared)
    for macro, value in (("CG1_FIXED_MAX_BASES", native_lib.FIXED_MAX_BASES), ("CG1_FIXED_MAX_MSMS", native_lib.FIXED_MAX_MSMS),
                         ("CG1_FIXED_MAX_TERMS", native_lib.FIXED_MAX_TERMS)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), src), macro
    assert native_lib.FIXED_MAX_MSMS >= 256 and native_lib.FIXED_MAX_TERMS >= 2048


def test_table_needs_a_gpu_and_leaves_random_alone(native_lib):
    """Without a GPU the constructor raises NativeError (no CPU fallback for an MSM); with one it builds.  Either way the module-level
    `random` state is untouched."""
    from curdleproofs_pie_amd import G1Point, Scalar
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable

    pts = [G1Point(), G1Point() * Scalar(5)]
    random.seed(99)
    state = random.getstate()
    if native_lib.cg1_device_count() <= 0:
        with pytest.raises(native_lib.NativeError):
            FixedBaseTable(pts)
    else:
        tab = FixedBaseTable(pts)
        assert len(tab) == 2 and tab.nbytes == 2 * 512 * 1024
        tab.close()
    assert random.getstate() == state
