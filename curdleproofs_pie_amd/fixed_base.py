"""MSMs over a resident table of fixed bases (csrc/kernels_fixed.h): the CRS points of the protocol, precomputed once.

    tab = FixedBaseTable(points)            # list of G1Point; deferred values are forced; the objects are held by identity
    tab.index(point)                        # position of that very object, KeyError otherwise
    tab.msm(scalars, bases=None)            # bases: G1Point objects of the table or indices; default = all, in order
    tab.msm_many([(bases, scalars), ...])   # one call, one launch chain -> [G1Point]
    tab.nbytes; tab.close()
    FixedBaseTable.for_crs(crs)             # vec_G | vec_H | H | G_t | G_u | G_sum | H_sum, the order of crs.py:92-101

Every MSM of a prover's halving rounds runs over `crs.vec_G`, `vec_H`, `H`, ... (prover_kernels.ipa_rounds_many keeps the bases fixed
and folds the challenges into the scalars), yet `compute_MSM` pays a full Pippenger pass with its doublings for them call after call.
A table holds the 32 x 128 multiples d * 2^(8 w) * B of every base (512 KiB each: 66.5 MiB for the 133 points of an ell = 124 CRS); a term
is then at most 32 additions and the sum is finished on the device.  There is no CPU path: without a GPU the constructor raises
`NativeError`, like every MSM of this package.

    lt = LightTable(points)                 # the same surface over a LIGHT table (csrc/kernels_light.h): for points that live for one
                                            # proof (vec_T, vec_U).  Built on the device in the constructor, 128 KiB per base, a term
                                            # is at most 64 additions
"""
from __future__ import annotations

import ctypes
import weakref
from array import array
from typing import Iterable, List, Sequence, Tuple, Union

from . import _native as N
from . import py_arkworks_bls12381 as B
from .py_arkworks_bls12381 import G1Point, Scalar, pack_scalars, points_from_blobs, points_to_affine96

_LOCK = B._LOCK                          # the Python face's one re-entrant lock (msm_accumulator.compute_MSM_batch runs under it too)
_tables: "weakref.WeakSet[FixedBaseTable]" = weakref.WeakSet()

Base = Union[G1Point, int]


class FixedBaseTable:
    """A table of fixed bases on the default context's GPU.  Thread-safe; freed at close(), at garbage collection and before
    N.close_default_context()."""

    _KIND, _MAX_BASES, _MAX_MSMS, _MAX_TERMS = "fixed-base", N.FIXED_MAX_BASES, N.FIXED_MAX_MSMS, N.FIXED_MAX_TERMS
    _create = staticmethod(lambda ctx, raw, n: ctx.fixed_table(raw, n))
    _native_msm = staticmethod(N.cg1_fixed_msm)

    def __init__(self, points: Iterable[G1Point]):
        with _LOCK:
            ctx = N.default_context()    # no GPU: NativeError here -- there is no CPU fallback for an MSM
            pts = list(points)
            if not 1 <= len(pts) <= self._MAX_BASES:
                raise ValueError(f"a {self._KIND} table holds 1 .. {self._MAX_BASES} points, not {len(pts)}")
            for p in pts:
                if type(p) is not G1Point:
                    raise TypeError(f"{type(self).__name__} takes G1Point objects")
            raw = points_to_affine96(pts)                     # forces deferred values, one shared inversion
            self._points = tuple(pts)                         # held: the identities below stay valid
            self._pos = {}
            for i, p in enumerate(pts):
                self._pos.setdefault(id(p), i)
            self._sg = [p._sg is True for p in pts]           # certified in G1? (unknown counts as no)
            self._all = array("I", range(len(pts)))
            self._ctx = ctx
            self._tab = self._create(ctx, raw, len(pts))
            _tables.add(self)

    @classmethod
    def for_crs(cls, crs) -> "FixedBaseTable":
        """vec_G | vec_H | H | G_t | G_u | G_sum | H_sum (crs.py:92-101): ell + n_blinders + 5 points."""
        return cls(list(crs.vec_G) + list(crs.vec_H) + [crs.H, crs.G_t, crs.G_u, crs.G_sum, crs.H_sum])

    def __len__(self) -> int:
        return len(self._points)

    @property
    def nbytes(self) -> int:
        """Device bytes of the table's records (0 once closed)."""
        return self._tab.nbytes if self._tab is not None else 0

    def index(self, point: G1Point) -> int:
        """Position of that very object in the table (identity, not equality): KeyError when it is not one of the table's."""
        try:
            return self._pos[id(point)]
        except KeyError:
            raise KeyError("not an object of this table") from None

    def close(self) -> None:
        with _LOCK:
            tab, self._tab = self._tab, None
            if tab is not None:
                tab.free()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ctx_lock(self):
        """The lock every call on this table's context runs under; raises when the table is closed."""
        if self._tab is None or not self._tab.handle or not self._ctx.handle:
            raise N.NativeError(f"the {self._KIND} table is closed")
        return _LOCK

    def _indices(self, bases: Sequence[Base], n: int):
        pos = self._pos
        m = len(self._points)
        out = array("I", bytes(4 * n))
        for i in range(n):
            b = bases[i]
            if type(b) is G1Point:
                j = pos.get(id(b))
                if j is None:
                    raise KeyError("a base is not an object of this table")
            else:
                j = int(b)
                if not 0 <= j < m:
                    raise IndexError(f"base index {j} outside the table of {m}")
            out[i] = j
        return out

    def msm(self, scalars: Sequence[Scalar], bases: Sequence[Base] = None) -> G1Point:
        """sum_i scalars[i] * bases[i]; bases default to the table's points in order (truncated to the shorter, like compute_MSM)."""
        return self.msm_many([(bases, scalars)])[0]

    def msm_many(self, jobs: Iterable[Tuple[Sequence[Base], Sequence[Scalar]]]) -> List[G1Point]:
        """[sum_i scalars[i] * bases[i] for (bases, scalars) in jobs] as ONE launch chain (k_table_msm with the table's plan).  bases: G1Point objects of the
        table or indices into it, None = the table in order.  A result is certified in G1 only when every base it used was."""
        with _LOCK:
            if self._tab is None or not self._tab.handle or not self._ctx.handle:
                raise N.NativeError(f"the {self._KIND} table is closed")
            idx = array("I")
            offsets = array("I", [0])
            all_sc: list = []
            certified = []
            sg = self._sg
            for bases, scalars in jobs:
                if not isinstance(scalars, (list, tuple)):
                    scalars = list(scalars)
                if bases is None:
                    n = min(len(scalars), len(self._points))
                    part = self._all[:n]
                else:
                    if not isinstance(bases, (list, tuple)):
                        bases = list(bases)
                    n = min(len(scalars), len(bases))
                    part = self._indices(bases, n)
                if n > self._MAX_TERMS:
                    raise ValueError(f"an MSM over a {self._KIND} table takes at most {self._MAX_TERMS} terms")
                idx.extend(part)
                all_sc.extend(scalars if len(scalars) == n else scalars[:n])
                offsets.append(len(idx))
                certified.append(all(sg[j] for j in part))
            m = len(offsets) - 1
            if m == 0:
                return []
            out: List[G1Point] = []
            for lo in range(0, m, self._MAX_MSMS):            # (more MSMs than one launch carries: several calls)
                hi = min(m, lo + self._MAX_MSMS)
                t0, t1 = offsets[lo], offsets[hi]
                nt = t1 - t0
                scb = ctypes.create_string_buffer(32 * max(nt, 1))
                pack_scalars(all_sc, ctypes.addressof(scb), nt, t0, nt)
                part_idx = idx[t0:t1] if (lo or hi != m) else idx
                offs = array("I", [o - t0 for o in offsets[lo: hi + 1]])
                blobs = ctypes.create_string_buffer(N.POINT_BYTES * (hi - lo))
                ia, _ = part_idx.buffer_info()
                oa, _ = offs.buffer_info()
                self._ctx.check(self._native_msm(self._ctx.handle, self._tab.handle, ia if nt else None, ctypes.addressof(scb), oa, hi - lo,
                                                ctypes.addressof(blobs), None))
                out.extend(points_from_blobs(blobs, hi - lo))
            for p, ok in zip(out, certified):
                if ok and p._sg is not True:
                    B._set(p, "_sg", True)
            return out


class LightTable(FixedBaseTable):
    """A LIGHT table (csrc/kernels_light.h) over points that live for one proof -- vec_T, vec_U -- with FixedBaseTable's whole surface
    (msm, msm_many, index, close, _indices, _ctx_lock): the two are interchangeable for callers.  Built on the device inside the
    constructor (two launches, 128 KiB per base instead of 512), a term costs up to 64 additions instead of 32."""

    _KIND, _MAX_BASES, _MAX_MSMS, _MAX_TERMS = "light", N.LIGHT_MAX_BASES, N.LIGHT_MAX_MSMS, N.LIGHT_MAX_TERMS
    _create = staticmethod(lambda ctx, raw, n: ctx.light_table(raw, n))
    _native_msm = staticmethod(N.cg1_light_msm)

    @classmethod
    def for_crs(cls, crs):
        raise TypeError("the CRS lives as long as the process: FixedBaseTable.for_crs(crs)")


def _close_all() -> None:
    for t in list(_tables):
        t.close()


N.on_close_default_context(_close_all)   # N.close_default_context() frees the tables made on it first
