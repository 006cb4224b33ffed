"""Self-overlap Q(t) and the four-point dynamic susceptibility chi_4(t) on MI355X, from positions.

    Q(t0, tau)  = sum_n Theta(a - |x_n(t0 + tau) - x_n(t0)|)              (the atoms that have moved less than a)
    q(tau)      = < Q(t0, tau) > / N
    chi_4(tau)  = ( < Q(t0, tau)^2 > - < Q(t0, tau) >^2 ) / N             (the averages over time origins t0)

chi_4 measures dynamic heterogeneity: it peaks near the structural relaxation time, where the atoms that have and have
not moved form the largest correlated domains.  It is a variance over origins, so the per-origin counts are what the
library computes (``k_overlap`` behind ``ta_overlap`` of ``include/ta_hip.h``, hand-written HIP: one pass over the
position slab per chunk of lags, integer counters in registers; a float32 slab is read as float32, never widened first)
-- Q adds up over atoms, Q^2 does not, so blocks of atoms on several devices or ranks are summed BEFORE the variance is
taken here, in float64 on the host.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from ._base import CollectiveAnalysis
from .vanhove import _VanHove, _check_lags, log_lags

#: TA_OVERLAP_MAX_CUTOFFS of include/ta_hip.h
MAX_CUTOFFS = 4


def _check_cutoffs(cutoff):
    a = np.atleast_1d(np.asarray(cutoff, dtype=np.float64))
    if a.ndim != 1 or not 1 <= a.size <= MAX_CUTOFFS:
        raise ValueError(f"cutoff: a scalar or a sequence of 1 ... {MAX_CUTOFFS} values is expected, got shape {a.shape}")
    if not np.all(np.isfinite(a)) or not np.all(a > 0) or np.any(np.diff(a) <= 0):
        raise ValueError(f"cutoff: finite, > 0 and strictly increasing values are expected, got {a.tolist()}")
    return np.ascontiguousarray(a)


class DynamicSusceptibility(CollectiveAnalysis):
    r"""Self-overlap and four-point susceptibility of a group of atoms (or of molecules' centres).

    .. math:: Q(t_0, \tau) = \sum_n \Theta(a - |\mathbf{x}_n(t_0 + \tau) - \mathbf{x}_n(t_0)|), \qquad
              q(\tau) = \frac{\langle Q \rangle}{N}, \qquad
              \chi_4(\tau) = \frac{\langle Q^2 \rangle - \langle Q \rangle^2}{N}

    with the averages over the :math:`T - \tau` time origins.  The comparison is strict: an atom exactly at distance a
    is not counted (``VanHoveSelf``'s bins are ``e[b] <= r2 < e[b + 1]``: with ``a = b dr`` the sum of Q over origins is
    the cumulative count of its bins below b, exactly).

    Two things to keep in mind when reading ``chi4``.  It is ensemble-dependent: this is the fluctuation at the
    trajectory's fixed N (and whatever else the simulation holds fixed), which is a lower bound of the susceptibility of
    an ensemble where those fluctuate.  And consecutive origins are correlated: the variance over all ``T - tau`` origins
    is the plain (``ddof=0``) one, not an estimate with ``T - tau`` independent samples; ``results.overlap_by_origin``
    is there for block averages and strides of one's own.

    Parameters
    ----------
    atomgroup : AtomGroup — the trajectory must hold positions.
    lags : integer frame lags, strictly increasing, below the number of analysed frames; ``None`` (the default):
        ``log_lags(n_frames, per_decade=8)``.
    cutoff : keyword-only — the overlap length a, a scalar or a strictly increasing sequence of up to 4 (one pass
        serves them all).
    dim_type : {'xyz', 'xy', 'yz', 'xz', 'x', 'y', 'z'}.
    unwrap : bool, default False — undo periodic wrapping first (``EinsteinMSD``'s); wrapped positions give wrong
        displacements.
    compound, compound_weights, reference_frame : keyword-only — as for ``VanHoveSelf``: the displacements of
        molecules' centres; N is then the number of compounds.
    device, devices, distributed, stage_dtype : keyword-only — as for the other classes.  float32 staging stays float32
        on the device (unless ``unwrap=True``, which works on float64 slabs).  Under ``distributed=True`` and
        ``devices=[...]`` the blocks' Q are added before any variance is taken.
    A box is needed only for ``unwrap``.  ``by_particle=True`` raises ``TypeError``.

    Attributes
    ----------
    results.lags (L,); results.times (L,) ps; results.cutoffs (C,); results.n_origins (L,) = T - lags;
    results.overlap_by_origin (C, L, T) int64, the raw Q, zeros at t0 >= T - lag; results.q (C, L) = mean over the valid
    origins of Q / N; results.chi4 (C, L) = the variance (``ddof=0``, two-pass) over the valid origins of Q, / N, NaN
    where there are fewer than two origins.  A scalar ``cutoff`` keeps the leading axis of length 1.
    """

    _accepts_compound = True
    _record_volumes = False
    _no_data_message = "Dynamic susceptibility computation requires positions in the trajectory"
    _updating_message = "UpdatingAtomGroups are not valid for dynamic susceptibility computation"
    _by_particle_message = ("DynamicSusceptibility has no per-particle result: the overlap is a sum over all atoms "
                            "(by_particle=True is not supported)")
    _result_keys = ("lags", "times", "cutoffs", "n_origins", "overlap_by_origin", "q", "chi4")

    def __init__(self, atomgroup, lags=None, *, cutoff, dim_type="xyz", unwrap=False, **kwargs):
        super().__init__(atomgroup, None, dim_type, None, False, unwrap, kwargs)
        self.cutoffs = _check_cutoffs(cutoff)
        self.lags = None if lags is None else _check_lags(lags)

    # the float32 rule and the data a frame must hold are the van Hove classes'
    _set_options = _VanHove._set_options
    _has_data = staticmethod(_VanHove._has_data)

    def _prepare(self):
        # (before the slabs are allocated: the number of analysed frames is known here, the trajectory is not read yet)
        if self.lags is None:
            self._lags = log_lags(self.n_frames)
            if self._lags.size == 0:
                raise ValueError(f"lags=None needs at least two analysed frames, got {self.n_frames}")
        else:
            self._lags = _check_lags(self.lags, self.n_frames)
        super()._prepare()
        for key in self._result_keys:
            setattr(self.results, key, None)

    def _moments(self, fft, lo, hi, correlate):
        return (self._ctx.overlap(self._lags, self.cutoffs),), None

    def _no_moments(self):
        return (np.zeros((self.cutoffs.size, self._lags.size, self.n_frames)),)

    def _correlate(self, fft, sums):
        return None  # the sums are the result: there is no correlation step

    def _store(self, sums, _):
        # (under distributed=True Q has travelled as float64 through the all-reduce: integers below 2^53 are exact there,
        # and an entry is at most N)
        Q = np.rint(sums[0]).astype(np.int64)
        r, T, N = self.results, self.n_frames, float(self.n_particles)
        r.lags = self._lags
        r.times = self._lags * (float(self.times[1] - self.times[0]) if T > 1 else 0.0)
        r.cutoffs = self.cutoffs
        r.n_origins = T - self._lags
        r.overlap_by_origin = Q
        r.q = np.empty(Q.shape[:2])
        r.chi4 = np.full(Q.shape[:2], np.nan)
        for l, n in enumerate(r.n_origins):
            valid = Q[:, l, :n].astype(np.float64)
            r.q[:, l] = valid.mean(axis=1) / N
            if n >= 2:
                r.chi4[:, l] = np.var(valid, axis=1) / N
