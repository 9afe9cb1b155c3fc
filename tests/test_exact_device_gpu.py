"""The two batch verifiers decide the proofs that carry a point outside G1 in ONE device pass (exact_device=True; k_exact_relations) or one by
one (exact_device=False, the path they always had): the same verdicts and status codes as the reference's, whatever the weights are.
  ShuffleBatchVerifier   tests/golden/torsion_vectors.json (ell = 12) and tests/golden/exact_device_vectors.json (ell = 4: T3 on each of the ten
                         watched points, cancelling torsion), both modes, weights all = 1 (mod 3), all = 0 (mod 3) and random
  OpeningBatchVerifier   the nine opening cases of torsion_vectors.json x 40
Needs an MI355X."""
import json
import os
import random

import pytest

from oracle import bls12_381 as O
from test_torsion import MultiplesOfThree, NeverMultiplesOfThree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def opening():
    """-> (items, the reference's verdicts, which proofs carry a decodable point outside G1)"""
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "torsion_vectors.json")))["opening"]
    assert len(t) == 9
    items = [((bytes.fromhex(c["r_G"]), bytes.fromhex(c["k_r_G"])), bytes.fromhex(c["k_commitment"]), bytes.fromhex(c["proof"])) for c in t]
    want = [c["accepts"] for c in t]
    flagged = []
    for (r, kr), k, pf in items:
        pts = [O.g1_decompress(e) for e in (r, kr, k, pf[:48], pf[48:96])]
        flagged.append(any(p is not None and not O.g1_in_subgroup(p) for p in pts))
    # a parity run cannot pass vacuously: both verdicts among the flagged proofs, and proofs that are not flagged
    assert sum(f and w for f, w in zip(flagged, want)) >= 2 and sum(f and not w for f, w in zip(flagged, want)) >= 2 and not all(flagged)
    return items, want, flagged


@pytest.fixture(scope="module")
def ctx(native_lib):
    cx = native_lib.Context(0)
    yield cx
    cx.close()


@pytest.mark.parametrize("device_front_end", [True, False])
def test_opening_flagged_proofs_on_the_device_and_on_the_host(native_lib, ctx, opening, device_front_end):
    from curdleproofs_pie_amd.shuffle_verifier import OpeningBatchVerifier

    items, want, flagged = opening
    batch, nflag = items * 40, 40 * sum(flagged)
    seen = {}
    for exact_device in (True, False, None):
        v = OpeningBatchVerifier(ctx, device_front_end=device_front_end, exact_device=exact_device)
        by_default = "device" if nflag >= v.EXACT_DEVICE_MIN else "host"
        for name, rng in (("= 1 mod 3", MultiplesOfThree()), ("= 0 mod 3", NeverMultiplesOfThree()), ("random", random.Random(5))):
            assert v.verify_many(batch, rng=rng) == want * 40, (exact_device, name)
            assert v.last_exact_path == {True: "device", False: "host", None: by_default}[exact_device]
            assert all((s == 0) == w for s, w in zip(v.last_status, want * 40))
            assert seen.setdefault(name, v.last_status) == v.last_status, (exact_device, name)      # the same codes on every path
        # one flagged proof among honest ones, from the first flagged proof on when forced; a batch without any reports no path
        one = [items[0]] * 7 + [items[flagged.index(True)]]
        assert v.verify_many(one) == [want[0]] * 7 + [want[flagged.index(True)]]
        assert v.last_exact_path == {True: "device", False: "host", None: "device" if 1 >= v.EXACT_DEVICE_MIN else "host"}[exact_device]
        assert v.verify_many([items[0], items[3]] * 4) == [True] * 8 and v.last_exact_path is None
        # the small path is untouched
        assert v.verify_many(items[:4]) == want[:4] and v.last_exact_path is None


def test_opening_device_pass_grows_its_buffers_once(native_lib, ctx, opening):
    from curdleproofs_pie_amd.shuffle_verifier import OpeningBatchVerifier

    items, want, flagged = opening
    v = OpeningBatchVerifier(ctx, exact_device=True)
    assert v.verify_many(items * 2) == want * 2
    kept = v._xdev
    assert v.verify_many(items * 20) == want * 20 and v._xdev is kept               # 80 flagged proofs fit the first allocation
    assert v.verify_many(items * 80) == want * 80 and v._xdev[0] >= 320 and v._xdev is not kept


# ---------------------------------------------------------------- ShuffleBatchVerifier
WATCHED_OFFSETS = lambda ell, lg: [4 * ell + 2 + j for j in range(6)] + [4 * ell + 12 + 4 * lg + j for j in range(4)]


def shuffle_fixture(name):
    """-> (crs bytes, items, the reference's verdicts, which proofs carry a watched point outside G1)"""
    sh = json.load(open(os.path.join(ROOT, "tests", "golden", name)))["shuffle"]
    tr = lambda r, k: [(r[i: i + 48], k[i: i + 48]) for i in range(0, len(r), 48)]
    items = [(tr(bytes.fromhex(c["pre_r"]), bytes.fromhex(c["pre_k"])), tr(bytes.fromhex(c["post_r"]), bytes.fromhex(c["post_k"])), bytes.fromhex(c["proof"]))
             for c in sh["cases"]]
    want = [c["accepts"] for c in sh["cases"]]
    ell = sh["ell"]
    lg = (ell + 4).bit_length() - 1
    flagged = []
    for _, _, proof in items:
        # the proof's points in wire order, the Fr fields skipped (M .. C, r_p | B_c B_d L/R_C L/R_D, c d | cm_A cm_B): positions from 4 ell on
        pos, off, enc = 4 * ell, 0, {}
        for run, skip in ((10, 1), (2 + 4 * lg, 2), (4, 3)):
            for _ in range(run):
                enc[pos] = proof[off: off + 48]
                pos, off = pos + 1, off + 48
            off += 32 * skip
        pts = [O.g1_decompress(enc[q]) for q in WATCHED_OFFSETS(ell, lg)]
        flagged.append(any(p is not None and not O.g1_in_subgroup(p) for p in pts))
    return bytes.fromhex(sh["crs"]), items, want, flagged


@pytest.fixture(scope="module")
def shuffles():
    fx = {name: shuffle_fixture(name) for name in ("torsion_vectors.json", "exact_device_vectors.json")}
    fa = sum(f and w for _, _, want, flagged in fx.values() for f, w in zip(flagged, want))
    fr = sum(f and not w for _, _, want, flagged in fx.values() for f, w in zip(flagged, want))
    assert fa >= 4 and fr >= 4, (fa, fr)                  # a parity run cannot pass vacuously
    assert sum(fx["exact_device_vectors.json"][3]) == 14 and sum(fx["torsion_vectors.json"][3]) == 4
    return fx


@pytest.mark.parametrize("mode", ["merged", "independent"])
@pytest.mark.parametrize("name", ["torsion_vectors.json", "exact_device_vectors.json"])
def test_shuffle_flagged_proofs_on_the_device_and_one_by_one(native_lib, shuffles, name, mode):
    from curdleproofs_pie_amd.shuffle_verifier import ShuffleBatchVerifier

    crs, items, want, flagged = shuffles[name]
    nflag = sum(flagged)
    clean = [it for it, f in zip(items, flagged) if not f]
    seen = {}
    for exact_device in (True, False):
        v = ShuffleBatchVerifier(crs, native_lib.Context(0), exact_device=exact_device)
        path = "device" if exact_device else "host"
        try:
            for wname, rng in (("= 1 mod 3", MultiplesOfThree()), ("= 0 mod 3", NeverMultiplesOfThree()), ("random", random.Random(7))):
                assert v.verify_many(items, mode=mode, rng=rng) == want, (exact_device, wname)
                assert all((s == 0) == w for s, w in zip(v.last_status, want))
                assert seen.setdefault(wname, v.last_status) == v.last_status, (exact_device, wname)      # the same codes on both paths
                assert v.last_stats["exact_checks"] == nflag and v.last_stats["exact_path"] == path
            calls = v.last_stats["exact_native_calls"]
            assert v.verify_many(items * 16, mode=mode) == want * 16
            assert v.last_stats["exact_checks"] == 16 * nflag and v.last_stats["exact_path"] == path
            if exact_device:
                assert v.last_stats["exact_native_calls"] == calls      # the native calls do not grow with the flagged count
            else:
                assert v.last_stats["exact_native_calls"] == 16 * calls
            assert v.verify_many(clean * 3, mode=mode) == [True] * (3 * len(clean))
            assert v.last_stats["exact_path"] is None and v.last_stats["exact_checks"] == 0 and v.last_stats["exact_native_calls"] == 0
        finally:
            v.close()


def test_shuffle_default_takes_the_device_pass_from_its_threshold(native_lib, shuffles):
    from curdleproofs_pie_amd.shuffle_verifier import ShuffleBatchVerifier

    crs, items, want, flagged = shuffles["exact_device_vectors.json"]
    v = ShuffleBatchVerifier(crs, native_lib.Context(0))
    try:
        m = v.EXACT_DEVICE_MIN
        one = [items[0]] * 5 + [items[flagged.index(True)]]
        assert v.verify_many(one) == [True] * 5 + [want[flagged.index(True)]]
        assert v.last_stats["exact_path"] == ("device" if 1 >= m else "host")
        reps = -(-m // sum(flagged))
        assert v.verify_many(items * reps) == want * reps and v.last_stats["exact_path"] == "device"
    finally:
        v.close()
