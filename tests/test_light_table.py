"""Light tables, the parts that run without a GPU: the signed narrow-window recoding the kernel computes (cg1_light_digits is compiled
from the function the kernel runs, csrc/light_digits.h), the symbol lists and limits, and the no-GPU failure mode of the Python class."""
import ctypes
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
LIGHT = ["cg1_light_create", "cg1_light_destroy", "cg1_light_len", "cg1_light_bytes", "cg1_light_msm", "cg1_light_msm_device", "cg1_light_digits"]


@pytest.fixture(scope="module")
def plan(native_lib):
    c = native_lib.LIGHT_WINDOW_BITS
    assert 3 <= c < 8
    return c, (256 + c - 1) // c


def digits(N, k, windows):
    out = (ctypes.c_int16 * (windows + 2))(*([0x5A5A] * (windows + 2)))
    assert N.cg1_light_digits(k.to_bytes(32, "little"), out) == windows
    assert out[windows] == 0x5A5A and out[windows + 1] == 0x5A5A          # nothing written past the plan's windows
    return list(out)[:windows]


def check(N, plan, k):
    c, windows = plan
    d = digits(N, k, windows)
    half = 1 << (c - 1)
    assert all(-half <= v <= half for v in d), (hex(k), d)
    assert sum(v << (c * w) for w, v in enumerate(d)) == k, (hex(k), d)
    return d


def test_digits_edge_scalars(native_lib, plan):
    c, windows = plan
    half = 1 << (c - 1)
    assert check(native_lib, plan, 0) == [0] * windows
    assert check(native_lib, plan, 1) == [1] + [0] * (windows - 1)
    check(native_lib, plan, R - 1)
    check(native_lib, plan, R - 2)
    assert check(native_lib, plan, half) == [half] + [0] * (windows - 1)            # 2^(c-1) stays a positive digit
    assert check(native_lib, plan, half + 1)[:2] == [-(half - 1), 1]                # 2^(c-1) + 1 = 2^c - (2^(c-1) - 1)
    for k in range(255):                                                            # 2^k and 2^k - 1: one digit / a carry chain from window 0
        check(native_lib, plan, 1 << k)
        d = check(native_lib, plan, (1 << k) - 1)
        if k and k % c == 0:
            assert d[0] == -1 and d[k // c] == 1 and not any(d[1: k // c])


def test_digits_carry_boundary(native_lib, plan):
    """Every window at the carry boundary: all digits 2^(c-1) (no carry anywhere), all 2^(c-1) + 1 (a carry out of every window), and
    runs of all-ones windows of every length at every position."""
    c, windows = plan
    half = 1 << (c - 1)
    top = 254 // c                                                                  # windows wholly below bit 254: the value stays below r
    for length in range(1, top + 1):
        k = sum(half << (c * w) for w in range(length))
        assert check(native_lib, plan, k)[:length] == [half] * length
        k = sum((half + 1) << (c * w) for w in range(length))
        if k < R:
            d = check(native_lib, plan, k)
            assert d[0] == -(half - 1) and all(v == -(half - 2) for v in d[1:length]) and d[length] == 1
    rng = random.Random(17)
    for start in range(0, top):
        for length in range(1, top - start + 1):
            k = ((1 << (c * length)) - 1) << (c * start)
            if k >= R:
                continue
            d = check(native_lib, plan, k)
            assert d[start] == -1 and d[start + length] == 1 and not any(d[start + 1: start + length])
            k2 = k | rng.getrandbits(c * start) if start else k
            if k2 < R:
                check(native_lib, plan, k2)
    # a carry into the top window that r allows: r's own top digits with everything below them set
    check(native_lib, plan, (R >> 200 << 200) - 1)
    check(native_lib, plan, (0x73 << 248) - 1)


def test_digits_random(native_lib, plan):
    rng = random.Random(18)
    for _ in range(2000):
        check(native_lib, plan, rng.randrange(R))


def test_symbols_and_limits(native_lib):
    N = native_lib
    src = open(os.path.join(ROOT, "include", "curdle_g1.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cg1_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in LIGHT:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in N.EXPORTED_SYMBOLS, name
        assert callable(getattr(N, name)), name
    for macro, value in (("CG1_LIGHT_WINDOW_BITS", N.LIGHT_WINDOW_BITS), ("CG1_LIGHT_MAX_BASES", N.LIGHT_MAX_BASES),
                         ("CG1_LIGHT_MAX_MSMS", N.LIGHT_MAX_MSMS), ("CG1_LIGHT_MAX_TERMS", N.LIGHT_MAX_TERMS)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), src), macro
    # the two plans of k_table_msm share the ticket words and slices; the prover's largest batch (64 provers, 2 n = 256 bases each) fits
    assert N.LIGHT_MAX_MSMS <= N.FIXED_MAX_MSMS and N.LIGHT_MAX_TERMS <= N.FIXED_MAX_TERMS and N.LIGHT_MAX_BASES >= 64 * 256
    assert N.cg1_light_len(None) == 0 and N.cg1_light_bytes(None) == 0
    N.cg1_light_destroy(None)


def test_table_needs_a_gpu_and_leaves_random_alone(native_lib):
    """Without a GPU the constructor raises NativeError (no CPU fallback for an MSM); with one it builds.  Either way the module-level
    `random` state is untouched."""
    from curdleproofs_pie_amd import G1Point, Scalar
    from curdleproofs_pie_amd.fixed_base import FixedBaseTable, LightTable

    assert issubclass(LightTable, FixedBaseTable)
    for name in ("msm", "msm_many", "close", "index", "_indices", "_ctx_lock"):
        assert callable(getattr(LightTable, name)), name
    pts = [G1Point(), G1Point() * Scalar(5)]
    random.seed(99)
    state = random.getstate()
    if native_lib.cg1_device_count() <= 0:
        with pytest.raises(native_lib.NativeError):
            LightTable(pts)
    else:
        c = native_lib.LIGHT_WINDOW_BITS
        tab = LightTable(pts)
        assert len(tab) == 2 and tab.nbytes == 2 * ((256 + c - 1) // c) * (1 << (c - 1)) * 256
        tab.close()
    assert random.getstate() == state
