"""Residence times in the solvation shell of a GROUP on MI355X, from positions: the residence-time function of Impey, Madden
and McDonald (MDAnalysis' ``SurvivalProbability`` with its ``intermittency``).  ``PairLifetime`` follows the indicator of one
pair (p, q): how long does THIS neighbour stay.  Here the indicator belongs to one observed item and is the OR over all
reference items,

    s_q(t) = [ some p in the reference group, p != q, with |x_q(t) - x_p(t)|_min.image < r_cut ],

so a molecule that slides from the shell of reference atom p1 into that of p2 without leaving the group's shell is ONE
residence, where every pair-resolved result counts two short ones.  One kernel (``k_shell_series`` behind
``ta_shell_residence`` of ``include/ta_hip.h``, hand-written HIP) forms the per-item level of every frame from an
all-against-all distance pass over ``VanHoveDistinct``'s gathered scratch and writes it in the layout of ``PairLifetime``'s
series block; hysteresis, the tolerated absence, the run lengths and the lag sums are ``PairLifetime``'s passes.  A float32
slab is read as float32, never widened first.  ``device="cpu"`` runs the opt-in CPU backend's twin (the same arithmetic, equal
counts); a GPU context never falls back to it.
"""
from __future__ import annotations

import warnings

import numpy as np

from ._lib import SHELL_CONDITIONS
from .pair_lifetime import PairLifetime, _trapezoid
from .vanhove_distinct import _sorted_ix

#: the library's cap on ``max_lag`` of the gated sums (eight passes of 256 lags)
MAX_LAG_CAP = 2047


class ShellResidence(PairLifetime):
    r"""Residence times of the observed atoms in the shell of a reference group.

    .. math:: R(\tau) = \frac{\sum_q \sum_{t < T - \tau} \prod_{s = t}^{t + \tau} g_q(s)}{\sum_q \sum_{t < T - \tau} g_q(t)}

    with :math:`g_q` the indicator :math:`s_q` after hysteresis (``r_break``) and the closing of absences of up to
    ``intermittency`` frames.  ``results.survival`` is this RATIO OF SUMS over all time origins.  MDAnalysis'
    ``SurvivalProbability`` averages the per-origin ratio :math:`N(t, t + \tau) / N(t)` over the origins instead; the two agree
    when the number of items inside, :math:`N(t)`, is constant, and differ otherwise (origins with many items inside weigh more
    here).  The per-origin form is not computed.

    Parameters
    ----------
    reference : AtomGroup — the group whose shell is meant (a solute, a polymer, a surface, all cations); the trajectory must
        hold positions.
    observed : AtomGroup or None — the atoms whose residence is followed; ``None``: the reference group itself ("in the shell of
        ANOTHER member": an atom is never in its own shell).  Two different groups must be disjoint.  The union is staged once.
    r_cut : keyword-only — the shell radius (strict: an atom exactly at ``r_cut`` is outside); with a box at most half of every
        analysed box length in every frame (``r_break`` where given).
    r_break : keyword-only, default None — a second, larger radius (hysteresis): an atom enters below ``r_cut`` and stays while
        SOME reference atom is closer than ``r_break``.  None: one radius.
    intermittency : keyword-only, default 0 — absences of at most this many frames (0 ... 63) between two frames inside count as
        inside, in every result: the tolerated absence t* of Impey's residence function.
    periodic, fft, dim_type, device, stage_dtype : keyword-only — as for ``PairLifetime``.

    ``devices=[...]`` with more than one member and ``distributed=True`` raise ``ValueError``; ``compound``,
    ``reference_frame``, ``unwrap`` and ``by_particle=True`` raise ``TypeError``.

    Attributes
    ----------
    results.times (T,) ps; results.n_inside (T,) int64 the observed atoms inside per frame; results.mean_inside its mean;
    results.run_lengths (T + 1,) int64 the number of residences of exactly l consecutive frames (the run open at the last frame
    ends there); results.survival (T,) = ``sum_{l > tau} run_lengths[l] (l - tau) / n0[tau]`` with ``n0[tau] = sum_{t < T -
    tau} n_inside[t]`` (see above: the ratio of sums); results.intermittent (T,) = ci / n0, inside at both ends whatever
    happened between; results.tau_residence, results.tau_intermittent their trapezoid integrals over times;
    results.mean_run the mean run length times dt.  Where no atom is ever inside these are ``nan`` (a warning).
    """

    _no_data_message = "Shell residence computation requires positions in the trajectory"
    _updating_message = "UpdatingAtomGroups are not valid for shell residence computation"
    _by_particle_message = ("ShellResidence has no per-particle result: the functions are sums over all observed atoms "
                            "(by_particle=True is not supported)")
    _result_keys = ("times", "n_inside", "mean_inside", "run_lengths", "survival", "intermittent", "tau_residence",
                    "tau_intermittent", "mean_run")

    def __init__(self, reference, observed=None, *, r_cut, r_break=None, intermittency=0, periodic=True, fft=True, dim_type="xyz",
                 **kwargs):
        for key in ("pairs", "search_stride"):
            if key in kwargs:
                raise TypeError(f"{type(self).__name__} does not take {key}=: every observed atom is followed against the whole reference "
                                "group, there is no list of pairs")
        self._refuse(kwargs, reference, observed)
        if observed is not None:
            ix_a, ix_b = _sorted_ix(reference, "reference"), _sorted_ix(observed, "observed")
            if not np.array_equal(ix_a, ix_b) and np.intersect1d(ix_a, ix_b).size:
                raise ValueError("reference and observed overlap but differ: they must be the same group or disjoint")
        super().__init__(reference, observed, r_cut=r_cut, periodic=periodic, fft=fft, dim_type=dim_type, r_break=r_break,
                         intermittency=intermittency, **kwargs)

    def _moments(self, fft, lo, hi, correlate):
        all_a = self.n_a == self.n_particles
        ci, runs, nb = self._ctx.shell_residence(fft, self.r_cut, r_break=self.r_break, gap=self.intermittency,
                                                 idx_a=None if all_a else self._idx_a, idx_b=None if self._same else self._idx_b,
                                                 dimensions=self._pair_boxes, axes=self._dim)
        return (ci, runs, nb), None

    def _store(self, sums, _):
        ci, runs, nb = sums
        r = self.results
        r.times = self.lag_times()
        r.n_inside = np.rint(nb).astype(np.int64)
        r.mean_inside = float(np.mean(r.n_inside))
        r.run_lengths = np.asarray(runs, dtype=np.int64)
        n0, cc, r.mean_run = self._run_sums(r.n_inside, r.run_lengths)
        if not r.n_inside.any():
            warnings.warn("ShellResidence: no observed atom is inside the shell in any frame; the residence functions are nan",
                          UserWarning, stacklevel=4)
        with np.errstate(divide="ignore", invalid="ignore"):
            r.intermittent = np.asarray(ci, dtype=np.float64) / n0
            r.survival = cc / n0.astype(np.float64)
        r.tau_intermittent = _trapezoid(r.intermittent, r.times)
        r.tau_residence = _trapezoid(r.survival, r.times)


class _GatedShell(ShellResidence):
    """What ShellMSD and ShellOrientation share: sums over the lags 0 ... ``max_lag`` whose terms are gated by the shell series
    under ``condition``, in the place of ShellResidence's lag sums."""

    _nothing_inside = None  # the warning where no series is ever inside, behind "<class name>: "

    def _refuse_fft(self, kwargs):
        if "fft" in kwargs:
            raise TypeError(f"{type(self).__name__} does not take fft=: the gate is a product over the frames between origin and lag, "
                            "there is no FFT form")

    @staticmethod
    def _check_condition(condition):
        if condition not in SHELL_CONDITIONS:
            raise ValueError(f"condition must be one of {sorted(SHELL_CONDITIONS)}, got {condition!r}")

    @staticmethod
    def _check_max_lag(max_lag):
        """max_lag as an int, or None"""
        if max_lag is None:
            return None
        if int(max_lag) != max_lag or max_lag < 0:
            raise ValueError(f"max_lag must be an integer >= 0, got {max_lag}")
        if max_lag > MAX_LAG_CAP:
            raise ValueError(f"max_lag must be at most {MAX_LAG_CAP}, got {max_lag}")
        return int(max_lag)

    def _prepare(self):
        if self.max_lag is not None and self.max_lag > self.n_frames - 1:
            raise ValueError(f"max_lag = {self.max_lag} needs more than the {self.n_frames} analysed frames")
        self._max_lag = min(self.n_frames - 1, 1024) if self.max_lag is None else self.max_lag
        super()._prepare()

    def _store_gated(self, sums):
        """times, count, n_inside, mean_inside, run_lengths and survival of the results; returns the gated sums (L + 1, n)"""
        S, count, runs, nb = sums
        r, L = self.results, self._max_lag
        r.times = self.lag_times()[:L + 1]
        r.count = np.asarray(count, dtype=np.int64)
        r.n_inside = np.rint(nb).astype(np.int64)
        r.mean_inside = float(np.mean(r.n_inside))
        r.run_lengths = np.asarray(runs, dtype=np.int64)
        n0 = np.cumsum(r.n_inside)[::-1][:L + 1].astype(np.float64)
        if not r.n_inside.any():  # (one frame further from the caller than a warning of _store's own)
            warnings.warn(f"{type(self).__name__}: {self._nothing_inside}", UserWarning, stacklevel=5)
        with np.errstate(divide="ignore", invalid="ignore"):
            r.survival = r.count / n0
        return np.asarray(S, dtype=np.float64)
