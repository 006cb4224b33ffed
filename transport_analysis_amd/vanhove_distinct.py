"""Distinct part of the van Hove function G_d(r, t) and the radial distribution function g(r) on MI355X, from positions.

    G_d(r, tau) = 1/Na < sum_{p in a} sum_{q in b, q != p} delta(r - |x_q(t0 + tau) - x_p(t0)|) >

averaged over time origins t0, with the minimum image of an orthorhombic box.  It is the real-space partner of the distinct
part of ``IntermediateScattering``'s F(k, t), and ``G_d(r, 0) / rho`` is the radial distribution function.  The cost is a
pair sum per origin and lag: a small gather pass (``k_vhd_gather``) turns the time-contiguous staged slab into frame-major
scratch, and the hot pass (``k_vhd_pairs`` behind ``ta_vanhove_distinct`` of ``include/ta_hip.h``, hand-written HIP) counts
the pair distances against squared bin edges in integer histograms.  A float32 slab is read as float32, never widened
first.  ``device="cpu"`` runs the opt-in CPU backend's twin of the two passes (the same arithmetic, equal counts); a GPU
context never falls back to it.
"""
from __future__ import annotations

import numpy as np

from ._base import UpdatingAtomGroup
from .vanhove import _VanHove, log_lags


def _sorted_ix(group, name):
    ix = getattr(group, "ix", None)
    if ix is None:
        ix = getattr(group, "indices", None)
    ix = np.asarray(ix, dtype=np.int64)
    if ix.ndim != 1 or ix.size == 0:
        raise ValueError(f"{name}: an AtomGroup with at least one atom is expected")
    out = np.unique(ix)
    if out.size != ix.size:
        raise ValueError(f"{name}: the group holds an atom more than once; a pair histogram counts every atom once")
    return out


class VanHoveDistinct(_VanHove):
    r"""Distinct van Hove function between two groups of atoms, with g(r) and the coordination number.

    .. math:: G_d(r, \tau) = \frac{1}{N_a\, n_\mathrm{orig}} \sum_{t_0} \sum_{p \in a} \sum_{q \in b,\, q \ne p}
              \delta(r - |\mathbf{x}_q(t_0 + \tau) - \mathbf{x}_p(t_0)|_\mathrm{min.\ image})

    Parameters
    ----------
    atomgroup : AtomGroup — the a-items (the centres); the trajectory must hold positions.
    atomgroup_b : AtomGroup or None — the b-items; ``None``: the same group (the like-like function).  The union of the two
        groups is staged once; an atom in both is never paired with itself.
    lags : integer frame lags, strictly increasing, below the number of analysed frames; default ``(0,)`` (the RDF alone);
        ``None``: ``(0,) + log_lags(n_frames)``.
    r_max, n_bins : keyword-only — ``n_bins`` bins of width ``dr = r_max / n_bins`` on [0, r_max); pairs beyond are counted in
        ``results.overflow``.  With a box ``r_max`` must not exceed half the shortest analysed box length.
    origin_stride : keyword-only — every ``origin_stride``-th analysed frame is a time origin.
    periodic : keyword-only, default True — use the minimum image of the frames' boxes (orthorhombic; constant unless
        every lag is 0).  False: plain distances, no box needed; ``g``, ``rdf`` and ``coordination`` are then ``None``.
    dim_type : {'xyz', 'xy', 'yz', 'xz', 'x', 'y', 'z'} — d, the number of analysed dimensions, follows.
    device, stage_dtype : keyword-only — as for the other classes.  float32 staging stays float32 on the device.

    Pair sums cross any split of the atoms: ``devices=[...]`` with more than one member and ``distributed=True`` raise
    ``ValueError``.  ``compound``, ``reference_frame``, ``unwrap`` (the minimum image makes unwrapping unnecessary) and
    ``by_particle=True`` raise ``TypeError``.

    Attributes
    ----------
    With ``n_origins[l] = ceil((T - lags[l]) / origin_stride)`` and the exact shell measures ``V_b`` of ``VanHoveSelf``:
    results.lags (L,); results.times (L,) ps; results.bin_edges (B + 1,); results.r (B,) the bin centres; results.counts
    (L, B) int64; results.overflow (L,); results.n_origins (L,); results.gd (L, B) = counts / (n_origins Na V_b);
    results.g (L, B) = gd / rho with rho = (Na Nb - \|a n b\|) / (Na <V>), which tends to 1 for uncorrelated positions;
    results.rdf (B,) the lag-0 row of g (``None`` if 0 is not among the lags); results.coordination (B,) the cumulative sum
    of the lag-0 counts over n_origins Na: the mean number of b-items within the bin's upper edge of an a-item.
    """

    _accepts_compound = False
    _record_volumes = True
    _by_particle_message = ("VanHoveDistinct has no per-particle result: the histograms are sums over all pairs "
                            "(by_particle=True is not supported)")
    _result_keys = ("lags", "times", "bin_edges", "r", "counts", "overflow", "n_origins", "gd", "g", "rdf", "coordination")

    def __init__(self, atomgroup, atomgroup_b=None, lags=(0,), *, r_max, n_bins=200, origin_stride=1, periodic=True,
                 dim_type="xyz", **kwargs):
        for key, why in (("compound", "pairs of atoms are counted, not of molecules' centres: run it on a group of one atom "
                                      "per molecule"),
                         ("compound_weights", "there are no compounds"),
                         ("reference_frame", "a pair distance does not depend on the frame of reference"),
                         ("unwrap", "the minimum image makes unwrapping unnecessary")):
            if kwargs.get(key) is not None and kwargs.get(key) is not False:
                raise TypeError(f"VanHoveDistinct does not take {key}=: {why}")
            kwargs.pop(key, None)
        devices = kwargs.get("devices")
        if devices is not None and len(list(devices)) > 1:
            raise ValueError("VanHoveDistinct: devices=[...] with more than one member is not supported -- the atoms would be "
                             "split over the GPUs by index, and the pair sums cross the shards")
        if kwargs.get("distributed", False):
            raise ValueError("VanHoveDistinct: distributed=True is not supported -- every rank holds a block of the atoms, and "
                             "the pair sums cross the blocks")
        if devices is not None:  # one member: a plain context on that device
            kwargs.pop("devices")
            kwargs.setdefault("device", list(devices)[0])
        if isinstance(atomgroup, UpdatingAtomGroup) or isinstance(atomgroup_b, UpdatingAtomGroup):
            raise TypeError(self._updating_message)
        same = atomgroup_b is None
        ix_a = _sorted_ix(atomgroup, "atomgroup")
        ix_b = ix_a if same else _sorted_ix(atomgroup_b, "atomgroup_b")
        union = np.union1d(ix_a, ix_b)
        # (the group itself where it already is the sorted union: its frames are then read without a gather)
        own = np.asarray(atomgroup.ix if hasattr(atomgroup, "ix") else atomgroup.indices)
        staged = atomgroup if np.array_equal(union, own) else atomgroup.universe.atoms[union]
        super().__init__(staged, lags, r_max, n_bins, dim_type, False, kwargs)
        self.group_a, self.group_b = atomgroup, atomgroup if same else atomgroup_b
        self._idx_a, self._idx_b = np.searchsorted(union, ix_a), np.searchsorted(union, ix_b)
        self.n_a, self.n_b = int(ix_a.size), int(ix_b.size)
        self.n_common = int(np.intersect1d(ix_a, ix_b).size)
        self.origin_stride = int(origin_stride)
        if self.origin_stride < 1:
            raise ValueError(f"origin_stride must be >= 1, got {origin_stride}")
        self.periodic = bool(periodic)

    def _default_lags(self):
        return np.concatenate([np.zeros(1, dtype=np.int64), log_lags(self.n_frames)])

    def _prepare(self):
        super()._prepare()
        self._pair_boxes = np.zeros((self.n_frames, 6)) if self.periodic else None

    def _single_frame(self):
        if self._pair_boxes is not None:
            ts = self._ts
            dims = ts.dimensions
            if dims is None:
                raise ValueError(f"periodic=True needs the periodic box, and frame {ts.frame} has none (ts.dimensions is None); "
                                 "pass periodic=False for plain distances")
            d = np.asarray(dims, dtype=np.float64).ravel()
            # (only the analysed axes: a slab geometry may have a zero length along an axis that is not analysed)
            if d.shape != (6,) or not np.all(np.isfinite(d)) or not np.all(d[list(self._dim)] > 0):
                raise ValueError(f"periodic=True needs box lengths > 0 on the analysed axes: frame {ts.frame} has dimensions {list(d)}")
            self._pair_boxes[self._frame_index] = d
        super()._single_frame()

    def _moments(self, fft, lo, hi, correlate):
        same = self.group_b is self.group_a
        all_a = self.n_a == self.n_particles
        counts = self._ctx.vanhove_distinct(self._lags, self.n_bins, self.dr, origin_stride=self.origin_stride,
                                            idx_a=None if all_a else self._idx_a,
                                            idx_b=None if same else self._idx_b,
                                            dimensions=self._pair_boxes, axes=self._dim)
        return (counts,), None

    def _no_moments(self):
        return (np.zeros((self._lags.size, self.n_bins + 1)),)

    def _store(self, sums, _):
        shell = self._store_grid(np.asarray(sums[0], dtype=np.int64))
        r, d = self.results, self.dim_fac
        r.n_origins = -(-(self.n_frames - self._lags) // self.origin_stride)
        norm = r.n_origins.astype(np.float64)[:, None] * float(self.n_a)
        r.gd = r.counts / (norm * shell[None, :])
        if not self.periodic:
            return
        # <V>: the measure of the analysed dimensions' cell (the volume, an area or a length), averaged over the frames
        cell = self._vol_avg if d == 3 else float(np.average(np.prod(self._pair_boxes[:, list(self._dim)], axis=1)))
        self.density = (float(self.n_a) * self.n_b - self.n_common) / (self.n_a * cell)
        r.g = r.gd / self.density
        zero = np.flatnonzero(self._lags == 0)
        if zero.size:
            r.rdf = r.g[zero[0]].copy()
            r.coordination = np.cumsum(r.counts[zero[0]]) / norm[zero[0], 0]
