"""Ion-pair, solvation-contact and hydrogen-bond lifetimes on MI355X, from positions: Rapaport's and Luzar-Chandler's pair
population correlation functions of the bond indicator ``h_pq(t) = [ |x_q(t) - x_p(t)|_min.image < r_cut ]``,

    C_I(tau) = < h(t0) h(t0 + tau) > / < h >                 intermittent: bonded at both ends, whatever happened between
    C_C(tau) = < h(t0) H(t0, tau) > / < h >                  continuous: bonded in EVERY frame from t0 to t0 + tau

over all candidate pairs and all time origins t0.  ``VanHoveDistinct`` tells where the neighbours are; this tells how long a
given neighbour stays.  The candidate pairs come from a pair-distance pass over ``VanHoveDistinct``'s gathered scratch
(``k_pair_find`` behind ``ta_pair_find`` of ``include/ta_hip.h``, hand-written HIP), or from an explicit list; a second pass
(``k_pair_series``) writes every candidate's 0/1 series as one more derived column of a pair-major block, C_I for every lag
at once is the VACF lag sum of that block, and C_C follows from the histogram of the lengths of the runs of bonded frames
(``k_pair_runs``): with every frame an origin, ``sum_t0 H(t0, tau) = sum_runs max(0, l - tau)``.  A float32 slab is read as
float32, never widened first.  ``device="cpu"`` runs the opt-in CPU backend's twin of the passes (the same arithmetic, equal
lists and counts); a GPU context never falls back to it.
"""
from __future__ import annotations

import warnings

import numpy as np

from ._base import CollectiveAnalysis, UpdatingAtomGroup
from .vanhove_distinct import _sorted_ix


def _trapezoid(y, t):
    return float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(t)))


class PairLifetime(CollectiveAnalysis):
    r"""Pair population correlation functions and lifetimes between two groups of atoms (or of an explicit list of pairs).

    .. math:: C_I(\tau) = \frac{\sum_{pq} \sum_{t < T - \tau} h_{pq}(t)\, h_{pq}(t + \tau)}{\sum_{pq} \sum_{t < T - \tau} h_{pq}(t)},
              \qquad C_C(\tau) = \frac{\sum_{pq} \sum_{t < T - \tau} \prod_{s = t}^{t + \tau} h_{pq}(s)}
              {\sum_{pq} \sum_{t < T - \tau} h_{pq}(t)}

    Parameters
    ----------
    atomgroup : AtomGroup — the a-items; the trajectory must hold positions.
    atomgroup_b : AtomGroup or None — the b-items; ``None``: the same group (unordered pairs, each counted once).  Two
        different groups must be disjoint.  The union of the groups is staged once.
    r_cut : keyword-only — the bond cutoff; with a box at most half of every analysed box length in every frame.
    pairs : keyword-only, (P, 2) integer array of ATOM indices (``atomgroup.ix`` values) or None — an explicit list of pairs that
        replaces the search (hydrogen-bond donor-acceptor lists, 1-4 pairs); ``atomgroup`` (with ``atomgroup_b``) must contain
        every atom named.  A pair named twice is counted twice.
    search_stride : keyword-only — every ``search_stride``-th analysed frame is searched for candidate pairs; a pair that is
        bonded only between searched frames is not a candidate.
    periodic : keyword-only, default True — use the minimum image of the frames' boxes (orthorhombic; they may change from
        frame to frame).  False: plain distances, no box needed.
    fft : keyword-only, default True — the lag sums by the FFT path (within 1e-10 of their largest value); False: the direct
        paths, exact integers.
    dim_type : {'xyz', 'xy', 'yz', 'xz', 'x', 'y', 'z'} — the analysed dimensions.
    r_break : keyword-only, default None — a second, larger cutoff (hysteresis, the stable-states picture): a bond forms below
        ``r_cut`` and lasts while the distance stays below ``r_break``.  None: one cutoff.
    intermittency : keyword-only, default 0 — absences of at most this many frames (0 ... 63) between two bonded frames count
        as bonded (MDAnalysis' ``intermittency``, the tolerated absence of residence times), in every result.  With either
        keyword set the series are filtered on the device (``ta_bond_lifetime``: ``k_bond_series``, ``k_pair_filter``); with
        the defaults nothing changes.
    device, stage_dtype : keyword-only — as for the other classes.  float32 staging stays float32 on the device.

    Pairs cross any split of the atoms: ``devices=[...]`` with more than one member and ``distributed=True`` raise
    ``ValueError``.  ``compound``, ``reference_frame``, ``unwrap`` (the minimum image makes unwrapping unnecessary) and
    ``by_particle=True`` raise ``TypeError``.

    Attributes
    ----------
    results.pairs (P, 2) atom indices of the candidate pairs, sorted by (a, b) when they were searched; results.times (T,) ps;
    results.n_bonded (T,) int64 the bonded pairs per frame; results.coordination the mean of n_bonded / Na;
    results.run_lengths (T + 1,) int64 the number of maximal runs of exactly l consecutive bonded frames (the distribution of
    bond durations; the run open at the last frame ends there); results.intermittent (T,) = ci / n0 with
    ``n0[tau] = sum_{t < T - tau} n_bonded[t]``; results.continuous (T,) = cc / n0 with ``cc[tau] = sum_{l > tau}
    run_lengths[l] (l - tau)``; results.tau_intermittent, results.tau_continuous their trapezoid integrals over times;
    results.mean_run the mean run length times dt.  Where no pair is ever bonded the correlations are ``nan`` (a warning).
    """

    _accepts_compound = False
    _record_volumes = False
    _no_data_message = "Pair lifetime computation requires positions in the trajectory"
    _updating_message = "UpdatingAtomGroups are not valid for pair lifetime computation"
    _by_particle_message = ("PairLifetime has no per-particle result: the correlations are sums over all pairs "
                            "(by_particle=True is not supported)")
    _n_at = 2  # items per row of the list, results.<_result_keys[0]>
    _staged_with = None  # universe indices staged along with the two groups (set by a subclass before __init__)
    _result_keys = ("pairs", "times", "n_bonded", "coordination", "run_lengths", "intermittent", "continuous",
                    "tau_intermittent", "tau_continuous", "mean_run")

    @staticmethod
    def _check_filters(r_cut, r_break, intermittency, name="r_break", cut_name="r_cut"):
        """(r_break or None, intermittency) of the two filter keywords, checked"""
        if r_break is not None:
            r_break = float(r_break)
            if not np.isfinite(r_break) or r_break < r_cut:
                raise ValueError(f"{name} must be finite and at least {cut_name}, got {r_break}")
        gap = int(intermittency)
        if gap != intermittency or not 0 <= gap <= 63:
            raise ValueError(f"intermittency must be an integer 0 ... 63 (frames of tolerated absence), got {intermittency}")
        return r_break, gap

    def _refuse(self, kwargs, *groups):
        """the keywords and groups this class and HydrogenBondLifetime cannot take; `kwargs` is left as the base class takes it"""
        name = type(self).__name__
        for key, why in (("compound", "pairs of atoms are followed, not of molecules' centres: run it on a group of one atom "
                                      "per molecule"),
                         ("compound_weights", "there are no compounds"),
                         ("reference_frame", "a pair distance does not depend on the frame of reference"),
                         ("unwrap", "the minimum image makes unwrapping unnecessary")):
            if kwargs.get(key) is not None and kwargs.get(key) is not False:
                raise TypeError(f"{name} does not take {key}=: {why}")
            kwargs.pop(key, None)
        devices = kwargs.get("devices")
        if devices is not None and len(list(devices)) > 1:
            raise ValueError(f"{name}: devices=[...] with more than one member is not supported -- the atoms would be "
                             "split over the GPUs by index, and the pairs cross the shards")
        if kwargs.get("distributed", False):
            raise ValueError(f"{name}: distributed=True is not supported -- every rank holds a block of the atoms, and "
                             "the pairs cross the blocks")
        if devices is not None:  # one member: a plain context on that device
            kwargs.pop("devices")
            kwargs.setdefault("device", list(devices)[0])
        if any(isinstance(g, UpdatingAtomGroup) for g in groups):
            raise TypeError(self._updating_message)

    def __init__(self, atomgroup, atomgroup_b=None, *, r_cut, pairs=None, search_stride=1, periodic=True, fft=True,
                 dim_type="xyz", r_break=None, intermittency=0, **kwargs):
        self._refuse(kwargs, atomgroup, atomgroup_b)
        self.r_cut = float(r_cut)
        if not np.isfinite(self.r_cut) or not self.r_cut > 0:
            raise ValueError(f"r_cut must be finite and > 0, got {r_cut}")
        self.search_stride = int(search_stride)
        if self.search_stride < 1:
            raise ValueError(f"search_stride must be >= 1, got {search_stride}")
        self.r_break, self.intermittency = self._check_filters(self.r_cut, r_break, intermittency)
        same = atomgroup_b is None
        ix_a = _sorted_ix(atomgroup, "atomgroup")
        ix_b = ix_a if same else _sorted_ix(atomgroup_b, "atomgroup_b")
        same = same or np.array_equal(ix_a, ix_b)
        if not same and np.intersect1d(ix_a, ix_b).size:
            raise ValueError("atomgroup and atomgroup_b overlap but differ: they must be the same group or disjoint (a pair "
                             "list counts every pair once)")
        union = np.union1d(ix_a, ix_b)
        if self._staged_with is not None:  # (atoms that are no items but are read with them: ShellOrientation's vectors)
            union = np.union1d(union, self._staged_with)
        # (the group itself where it already is the sorted union: its frames are then read without a gather)
        own = np.asarray(atomgroup.ix if hasattr(atomgroup, "ix") else atomgroup.indices)
        staged = atomgroup if np.array_equal(union, own) else atomgroup.universe.atoms[union]
        super().__init__(staged, None, dim_type, None, bool(fft), False, kwargs)
        self.group_a, self.group_b = atomgroup, atomgroup if same else atomgroup_b
        self._union, self._same = union, same
        self._idx_a, self._idx_b = np.searchsorted(union, ix_a), np.searchsorted(union, ix_b)
        self.n_a, self.n_b = int(ix_a.size), int(ix_b.size)
        self.periodic = bool(periodic)
        self._pairs = None
        if pairs is not None:
            p = np.asarray(pairs)
            if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1 or not np.issubdtype(p.dtype, np.integer):
                raise ValueError(f"pairs: a non-empty integer (P, 2) array of atom indices is expected, got shape {p.shape} and "
                                 f"dtype {p.dtype}")
            at = np.searchsorted(union, p)
            if np.any(at >= union.size) or np.any(union[np.minimum(at, union.size - 1)] != p):
                missing = p[(at >= union.size) | (union[np.minimum(at, union.size - 1)] != p)]
                raise ValueError(f"pairs: atom {int(missing[0])} is not in atomgroup; the group must contain every atom named")
            if np.any(p[:, 0] == p[:, 1]):
                raise ValueError(f"pairs: row {int(np.flatnonzero(p[:, 0] == p[:, 1])[0])} names an atom twice")
            self._pairs = np.ascontiguousarray(at, dtype=np.int32)

    def _set_options(self, dtype):
        # float32 staging stays float32 on the device: the kernels read it as it is
        self._ctx.set_option("stage_device_f32", int(dtype == np.float32))

    @staticmethod
    def _has_data(ts):
        return ts.has_positions

    def _prepare(self):
        super()._prepare()
        for key in self._result_keys:
            setattr(self.results, key, None)
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
        box = dict(dimensions=self._pair_boxes, axes=self._dim)
        staged = self._pairs
        if staged is None:
            all_a = self.n_a == self.n_particles
            staged = self._ctx.pair_find(self.r_cut, search_stride=self.search_stride, idx_a=None if all_a else self._idx_a,
                                         idx_b=None if self._same else self._idx_b, **box)
            if staged.shape[0] == 0:
                return self._no_moments() + (staged,), None
        if self.r_break is not None or self.intermittency:  # the filtered series: ta_bond_lifetime on rows of two items
            ci, runs, nb = self._ctx.bond_lifetime(fft, staged, self.r_cut, r_break=self.r_break, gap=self.intermittency, **box)
        else:  # (a searched list is the one the search left in the context)
            ci, runs, nb = self._ctx.pair_lifetime(fft, self.r_cut, None if self._pairs is None else staged, **box)
        return (ci, runs, nb, staged), None

    def _no_moments(self):
        T = self.n_frames
        return np.zeros(T), np.zeros(T + 1, dtype=np.int64), np.zeros(T)

    def _correlate(self, fft, sums):
        return None  # the sums are the result: there is no correlation step

    def _run_sums(self, n_in, run_lengths):
        """(n0, cc, mean_run) of the bonded (inside) counts per frame and the run-length histogram: n0[tau] = sum_{t < T - tau}
        n_in[t], cc[tau] = sum_{l > tau} run_lengths[l] (l - tau), suffix sums in int64; the mean run length times dt"""
        T = self.n_frames
        n0 = np.cumsum(n_in)[::-1].copy()
        ell = np.arange(T + 1, dtype=np.int64)
        s0 = np.cumsum(run_lengths[::-1])[::-1]          # s0[k] = sum_{l >= k} runs[l]
        s1 = np.cumsum((ell * run_lengths)[::-1])[::-1]  # s1[k] = sum_{l >= k} l runs[l]
        cc = s1[1:] - ell[:T] * s0[1:]
        n_runs = int(run_lengths.sum())
        dt = float(self.times[1] - self.times[0]) if T > 1 else 0.0
        return n0, cc, float(s1[0]) / n_runs * dt if n_runs else float("nan")

    def _store(self, sums, _):
        ci, runs, nb, staged = sums
        r = self.results
        setattr(r, self._result_keys[0], self._union[np.asarray(staged, dtype=np.int64)].reshape(-1, self._n_at))
        r.times = self.lag_times()
        r.n_bonded = np.rint(nb).astype(np.int64)
        r.coordination = float(np.mean(r.n_bonded / float(self.n_a)))
        r.run_lengths = np.asarray(runs, dtype=np.int64)
        n0, cc, r.mean_run = self._run_sums(r.n_bonded, r.run_lengths)
        if not r.n_bonded.any():
            warnings.warn(f"{type(self).__name__}: no pair is bonded in any frame; the correlation functions are nan", UserWarning,
                          stacklevel=4)
        with np.errstate(divide="ignore", invalid="ignore"):
            r.intermittent = np.asarray(ci, dtype=np.float64) / n0
            r.continuous = cc / n0.astype(np.float64)
        r.tau_intermittent = _trapezoid(r.intermittent, r.times)
        r.tau_continuous = _trapezoid(r.continuous, r.times)
