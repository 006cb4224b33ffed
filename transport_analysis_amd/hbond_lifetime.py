"""Hydrogen-bond lifetimes on MI355X: ``PairLifetime``'s population correlation functions of donor-hydrogen-acceptor triplets
with the geometric criterion of MDAnalysis' ``HydrogenBondAnalysis``,

    bonded(t) = |x_A - x_D|_min.image < d_a_cutoff  and  angle(D-H-A) >= d_h_a_angle_cutoff,

optionally with a looser break criterion (``d_a_break``, ``angle_break``: a bond forms by the first and lasts by the second)
and ``intermittency`` frames of tolerated absence.  The donor-hydrogen pairs come from a list or from one ``ta_pair_find`` on
the first frame, the donor-acceptor candidates from ``ta_pair_find`` at ``d_a_cutoff``; the triplets are expanded on the host
and ``ta_bond_lifetime`` (``k_bond_series``, ``k_pair_filter``, then ``PairLifetime``'s passes) does the rest on the device.
"""
from __future__ import annotations

import numpy as np

from ._base import CollectiveAnalysis
from .pair_lifetime import PairLifetime
from .vanhove_distinct import _sorted_ix


def _cosine(angle, name):
    """the cosine of an angle of 90 ... 180 degrees, inside [-1, 0]"""
    angle = float(angle)
    if not 90.0 <= angle <= 180.0:
        raise ValueError(f"{name} must lie in 90 ... 180 degrees, got {angle}")
    return min(0.0, max(-1.0, float(np.cos(np.deg2rad(angle)))))


class HydrogenBondLifetime(PairLifetime):
    r"""Hydrogen-bond population correlation functions and lifetimes of donor-hydrogen-acceptor triplets.

    Parameters
    ----------
    donors, hydrogens, acceptors : AtomGroup — the three groups; their union is staged once.  Donors and acceptors are the
        same group (water: both directions of every pair are followed) or disjoint; hydrogens are disjoint from both.
    d_a_cutoff, d_h_a_angle_cutoff : keyword-only — a bond forms below this donor-acceptor distance with at least this
        D-H-A angle in degrees (90 ... 180; exactly on the angle counts as bonded, exactly on the distance does not).
    d_a_break, angle_break : keyword-only, default None — the break criterion (``d_a_break >= d_a_cutoff``,
        ``angle_break <= d_h_a_angle_cutoff``): a formed bond lasts while it holds.  None: the form value.
    donor_hydrogen_pairs : keyword-only, (n, 2) atom indices (donor, hydrogen) or None — None: every donor-hydrogen pair
        closer than ``d_h_cutoff`` in the FIRST analysed frame.
    intermittency, search_stride, periodic, fft, dim_type, device, stage_dtype : as for ``PairLifetime``.

    ``devices=[...]`` with more than one member, ``distributed=True``, ``compound``, ``reference_frame``, ``unwrap`` and
    ``by_particle=True`` are refused as by ``PairLifetime``.

    Attributes
    ----------
    results.bonds (P, 3) atom indices (donor, hydrogen, acceptor) of the candidate triplets; every other key as
    ``PairLifetime``'s, of the triplets; results.coordination is per donor.
    """

    _no_data_message = "Hydrogen bond lifetime computation requires positions in the trajectory"
    _updating_message = "UpdatingAtomGroups are not valid for hydrogen bond lifetime computation"
    _by_particle_message = ("HydrogenBondLifetime has no per-particle result: the correlations are sums over all triplets "
                            "(by_particle=True is not supported)")
    _n_at = 3
    _result_keys = ("bonds",) + PairLifetime._result_keys[1:]

    def __init__(self, donors, hydrogens, acceptors, *, d_a_cutoff=3.0, d_h_a_angle_cutoff=150.0, d_a_break=None, angle_break=None,
                 donor_hydrogen_pairs=None, d_h_cutoff=1.2, intermittency=0, search_stride=1, periodic=True, fft=True,
                 dim_type="xyz", **kwargs):
        self._refuse(kwargs, donors, hydrogens, acceptors)
        self.r_cut = float(d_a_cutoff)
        if not np.isfinite(self.r_cut) or not self.r_cut > 0:
            raise ValueError(f"d_a_cutoff must be finite and > 0, got {d_a_cutoff}")
        self.d_h_cutoff = float(d_h_cutoff)
        if not np.isfinite(self.d_h_cutoff) or not self.d_h_cutoff > 0:
            raise ValueError(f"d_h_cutoff must be finite and > 0, got {d_h_cutoff}")
        self.search_stride = int(search_stride)
        if self.search_stride < 1:
            raise ValueError(f"search_stride must be >= 1, got {search_stride}")
        self.r_break, self.intermittency = self._check_filters(self.r_cut, d_a_break, intermittency, "d_a_break", "d_a_cutoff")
        self.cos_cut = _cosine(d_h_a_angle_cutoff, "d_h_a_angle_cutoff")
        self.cos_break = self.cos_cut if angle_break is None else _cosine(angle_break, "angle_break")
        if self.cos_break < self.cos_cut:
            raise ValueError(f"angle_break must be at most d_h_a_angle_cutoff, got {angle_break} against {d_h_a_angle_cutoff}")
        ix_d, ix_h, ix_a = (_sorted_ix(g, n) for g, n in ((donors, "donors"), (hydrogens, "hydrogens"), (acceptors, "acceptors")))
        same = np.array_equal(ix_d, ix_a)
        if not same and np.intersect1d(ix_d, ix_a).size:
            raise ValueError("donors and acceptors overlap but differ: they must be the same group or disjoint (a pair "
                             "list counts every pair once)")
        if np.intersect1d(ix_h, np.union1d(ix_d, ix_a)).size:
            raise ValueError("hydrogens must be disjoint from donors and acceptors")
        union = np.union1d(np.union1d(ix_d, ix_a), ix_h)
        CollectiveAnalysis.__init__(self, donors.universe.atoms[union], None, dim_type, None, bool(fft), False, kwargs)
        self._union, self._same = union, same
        self._idx_d, self._idx_h, self._idx_a = (np.searchsorted(union, ix) for ix in (ix_d, ix_h, ix_a))
        self.n_a = int(ix_d.size)  # (coordination is per donor)
        self.periodic = bool(periodic)
        self._dh = None
        if donor_hydrogen_pairs is not None:
            p = np.asarray(donor_hydrogen_pairs)
            if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1 or not np.issubdtype(p.dtype, np.integer):
                raise ValueError(f"donor_hydrogen_pairs: a non-empty integer (n, 2) array of atom indices is expected, got shape "
                                 f"{p.shape} and dtype {p.dtype}")
            if not np.all(np.isin(p[:, 0], ix_d)) or not np.all(np.isin(p[:, 1], ix_h)):
                raise ValueError("donor_hydrogen_pairs: every row must name an atom of donors and an atom of hydrogens")
            self._dh = np.searchsorted(union, p)

    def _triplets(self, dh, da):
        """the rows (d, h, a) of staged ids: every found donor-acceptor pair with every hydrogen of its donor, in the order of
        `da`; donors == acceptors: the pair (a, b) is followed by (b, a)"""
        dh = dh[np.argsort(dh[:, 0], kind="stable")]
        first = np.searchsorted(dh[:, 0], np.arange(self.n_particles + 1))  # the hydrogens of item d: dh[first[d]:first[d + 1], 1]
        if self._same:
            da = np.stack([da, da[:, ::-1]], axis=1).reshape(-1, 2)
        n_h = first[da[:, 0] + 1] - first[da[:, 0]]
        row = np.repeat(np.arange(da.shape[0]), n_h)
        k = np.arange(row.size) - np.repeat(np.cumsum(n_h) - n_h, n_h)  # which hydrogen of the row's donor
        out = np.stack([da[row, 0], dh[first[da[row, 0]] + k, 1], da[row, 1]], axis=1)
        return np.ascontiguousarray(out, dtype=np.int32)

    def _moments(self, fft, lo, hi, correlate):
        box = dict(dimensions=self._pair_boxes, axes=self._dim)
        dh = self._dh
        if dh is None:  # stride n_frames: frame 0 is the only searched frame
            dh = self._ctx.pair_find(self.d_h_cutoff, search_stride=self.n_frames, idx_a=self._idx_d, idx_b=self._idx_h, **box)
        da = self._ctx.pair_find(self.r_cut, search_stride=self.search_stride, idx_a=self._idx_d,
                                 idx_b=None if self._same else self._idx_a, **box)
        bonds = self._triplets(np.asarray(dh, dtype=np.int64), np.asarray(da, dtype=np.int64))
        if bonds.shape[0] == 0:
            return self._no_moments() + (bonds,), None
        ci, runs, nb = self._ctx.bond_lifetime(fft, bonds, self.r_cut, r_break=self.r_break, cos_cut=self.cos_cut,
                                               cos_break=self.cos_break, gap=self.intermittency, **box)
        return (ci, runs, nb, bonds), None
