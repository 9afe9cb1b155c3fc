"""Writes whisk_shuffle_seeded_vectors.json: what a seed draws for a Whisk shuffle, by hashlib alone.

    python tests/golden/gen_whisk_shuffle_seeded.py

The file fixes the FORMAT: a change of the domain string, the field order, the byte order or the reduction shows as a difference from it.
"""
import hashlib
import json
import os

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
FIELDS = (("k", 1), ("vec_m_blinders", 4), ("vec_a_blinders", 2), ("vec_c_blinders", 4), ("ipa_r", "n"), ("ipa_z_head", "n - 2"), ("r_t", 1), ("r_u", 1), ("r_a", 1),
          ("r_b", 1), ("r_k", 1), ("vec_r", "n"))


def block(seed, index, d):
    return hashlib.shake_256(b"whisk_shuffle_draw" + seed + index.to_bytes(8, "little") + d.to_bytes(4, "little")).digest(64)


def draws(seed, index, ell):
    n = ell + 4
    perm = list(range(ell))
    for d in range(ell - 1):
        i = ell - 1 - d
        j = int.from_bytes(block(seed, index, d)[:16], "little") % (i + 1)
        perm[i], perm[j] = perm[j], perm[i]
    d = ell - 1
    out = {"permutation": perm}
    for name, count in FIELDS:
        m = {"n": n, "n - 2": n - 2}.get(count, count)
        vals = []
        for _ in range(m):
            vals.append((int.from_bytes(block(seed, index, d), "little") % R).to_bytes(32, "little").hex())
            d += 1
        out[name] = vals if name.startswith(("vec_", "ipa_")) else vals[0]
    assert d == ell + 3 * n + 13
    return out


def main():
    cases = []
    for seed, index, ell in ((bytes(range(32)), 0, 4), (bytes(range(32)), 7, 12), (hashlib.sha256(b"whisk shuffle seeded").digest(), (1 << 32) - 1, 4),
                             (hashlib.sha256(b"whisk shuffle seeded").digest(), 1 << 31, 12)):
        cases.append({"seed": seed.hex(), "index": index, "ell": ell, **draws(seed, index, ell)})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "whisk_shuffle_seeded_vectors.json")
    with open(path, "w") as f:
        json.dump({"format": "SHAKE256(b'whisk_shuffle_draw' || seed || le64(index) || le32(d)).digest(64); scalars as 32 little-endian bytes, hex", "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
