"""The seeded draws of a Whisk shuffle written out with hashlib alone -- no product code -- and laid out as the
native entries return them.  Shared by tests/test_whisk_shuffle_seeded.py (the Python model, the golden file, the host twin) and
tests/test_whisk_shuffle_seeded_gpu.py (the device kernels, the whole call)."""
import functools
import hashlib

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
NB = 4
SEED_A = bytes(range(32))
SEED_B = hashlib.sha256(b"another seed").digest()


def block(seed, index, d):
    msg = b"whisk_shuffle_draw" + seed + index.to_bytes(8, "little") + d.to_bytes(4, "little")
    assert len(msg) == 62
    return hashlib.shake_256(msg).digest(64)


@functools.lru_cache(maxsize=None)
def model(seed, index, ell):
    """-> (permutation, [the 3 n + 14 scalars as ints, in draw order])"""
    n = ell + NB
    perm = list(range(ell))
    for d in range(ell - 1):
        i = ell - 1 - d
        j = int.from_bytes(block(seed, index, d)[:16], "little") % (i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    return perm, [int.from_bytes(block(seed, index, d), "little") % R for d in range(ell - 1, ell + 3 * n + 13)]


def widths(ell):
    """rows of the columns k | vec_m_blinders | vec_a_blinders | vec_c_blinders | ipa_r | ipa_z_head | r_t .. r_k | vec_r"""
    n = ell + NB
    return (1, NB, 2, NB, n, n - 2, 5, n)


def as_item(perm, scalars, ell):
    """the model's draws in the shape shuffle_draws_from_seed returns"""
    s32 = [v.to_bytes(32, "little") for v in scalars]
    cut, at = [], 0
    for w in widths(ell):
        cut.append(s32[at: at + w])
        at += w
    assert at == len(s32)
    k, mbl, abl, cbl, ipa_r, z_head, five, vec_r = cut
    return perm, k[0], mbl, (abl, cbl, ipa_r, z_head, *five, vec_r)


def columns(seed, first_index, ell, count):
    """what the native draw entries write for `count` shuffles: (perm as a flat list, the scalars in the column layout as bytes)"""
    models = [model(seed, first_index + p, ell) for p in range(count)]
    perm = [m for pm, _ in models for m in pm]
    out, at = [], 0
    for w in widths(ell):
        for _, sc in models:
            out += sc[at: at + w]
        at += w
    return perm, b"".join(v.to_bytes(32, "little") for v in out)
