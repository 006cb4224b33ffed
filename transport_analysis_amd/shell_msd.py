"""Mean squared displacement of atoms WHILE they stay in the solvation shell of a group on MI355X, from positions: the local,
shell-resolved diffusion of Liu, Harder and Berne (MDAnalysis' ``waterdynamics.MeanSquareDisplacement`` for a selection zone).
``ShellResidence`` answers how long an atom stays in the shell; this class answers how fast it moves while it is there.  The
indicator g_q(t) is ``ShellResidence``'s, bit for bit (``r_break`` hysteresis, tolerated absence), formed by the same passes;
one more kernel (``k_shell_msd`` behind ``ta_shell_msd`` of ``include/ta_hip.h``, hand-written HIP) adds up the squared
displacements over the lags 0 ... ``max_lag``, every term gated by bits of g, reading the staged slab in its own element type.
``device="cpu"`` runs the opt-in CPU backend's twin (the same arithmetic); a GPU context never falls back to it.
"""
from __future__ import annotations

import numpy as np

from .shell_residence import MAX_LAG_CAP, _GatedShell  # noqa: F401  (MAX_LAG_CAP: this module's name for it stays)


class ShellMSD(_GatedShell):
    r"""MSD of the observed atoms while they are in the shell of a reference group.

    .. math:: MSD_j(\tau) = \frac{\sum_q \sum_{t < T - \tau} w_q(t, \tau) (x_{q,j}(t + \tau) - x_{q,j}(t))^2}
              {\sum_q \sum_{t < T - \tau} w_q(t, \tau)}

    with :math:`w = \prod_{s = t}^{t + \tau} g_q(s)` for ``condition="continuous"`` (inside in every frame from t to t + tau)
    and :math:`w = g_q(t) g_q(t + \tau)` for ``condition="endpoints"`` (inside at both ends, whatever happened between:
    MDAnalysis waterdynamics' zone MSD).  g is ``ShellResidence``'s indicator after ``r_break`` and ``intermittency``.  The
    ratio is one of sums over all time origins; the per-origin ratio of means is not computed.  No fit is offered: as with
    ``EinsteinMSD`` the slope is the user's.

    The displacement is the plain difference of the staged positions (float64, no image): positions must be unwrapped.
    ``unwrap=True`` unwraps the staged slab on the device first (``ta_unwrap``, MDAnalysis' ``NoJump``; see ``EinsteinMSD``
    for its rules: every analysed frame needs a box, frames that are not consecutive give a ``UserWarning``, the device slab
    is then float64 whatever ``stage_dtype``).  ``ta_unwrap`` subtracts whole boxes OF THAT FRAME, x_u(t) = x(t) - n(t) H(t),
    so the distance pass that forms g, which keeps its ``rint`` minimum image, gives the same g on the unwrapped slab as on
    the wrapped one, for constant and per-frame orthorhombic boxes.

    Parameters
    ----------
    reference, observed, r_cut, r_break, intermittency, periodic, dim_type, device, stage_dtype : as for ``ShellResidence``.
    max_lag : keyword-only, default None — the largest lag in frames, 0 ... n_frames - 1 and at most 2047; ``None``:
        ``min(n_frames - 1, 1024)``.
    condition : keyword-only, ``"continuous"`` (default) or ``"endpoints"``.
    unwrap : keyword-only, default False — see above.

    ``fft=``, ``compound``, ``reference_frame`` and ``by_particle=True`` raise ``TypeError``; ``devices=[...]`` with more than
    one member and ``distributed=True`` raise ``ValueError``.

    Attributes
    ----------
    results.times (L + 1,) ps the lag times; results.count (L + 1,) int64 the terms N(tau); results.msd_axes (L + 1, D) the sums
    over N per analysed axis; results.msd (L + 1,) its row sums; a lag with count 0 has ``nan`` in both.  results.n_inside,
    results.mean_inside, results.run_lengths as ``ShellResidence``'s; results.survival (L + 1,) = ``count / n0`` with ``n0[tau] =
    sum_{t < T - tau} n_inside[t]``: under "continuous" ``ShellResidence``'s survival cut at L, under "endpoints" its
    ``intermittent``.  Where no atom is ever inside: ``nan`` (a warning).
    """

    _no_data_message = "Shell MSD computation requires positions in the trajectory"
    _updating_message = "UpdatingAtomGroups are not valid for shell MSD computation"
    _by_particle_message = ("ShellMSD has no per-particle result: the sums run over all observed atoms "
                            "(by_particle=True is not supported)")
    _result_keys = ("times", "count", "msd_axes", "msd", "n_inside", "mean_inside", "run_lengths", "survival")
    _nothing_inside = "no observed atom is inside the shell in any frame; the MSD is nan"

    def __init__(self, reference, observed=None, *, r_cut, r_break=None, intermittency=0, max_lag=None, condition="continuous",
                 unwrap=False, periodic=True, dim_type="xyz", **kwargs):
        self._refuse_fft(kwargs)
        self._check_condition(condition)
        max_lag = self._check_max_lag(max_lag)
        super().__init__(reference, observed, r_cut=r_cut, r_break=r_break, intermittency=intermittency, periodic=periodic,
                         fft=False, dim_type=dim_type, **kwargs)
        self.max_lag, self.condition = max_lag, condition
        self._unwrap = self.unwrap = bool(unwrap)

    def _set_options(self, dtype):
        # float32 staging stays float32 on the device: the kernels read it as it is (the unwrap pass works on float64 slabs)
        self._ctx.set_option("stage_device_f32", int(dtype == np.float32 and not self._unwrap))

    def _moments(self, fft, lo, hi, correlate):
        all_a = self.n_a == self.n_particles
        out = self._ctx.shell_msd(self.condition, self._max_lag, self.r_cut, r_break=self.r_break, gap=self.intermittency,
                                  idx_a=None if all_a else self._idx_a, idx_b=None if self._same else self._idx_b,
                                  dimensions=self._pair_boxes, axes=self._dim)
        return out, None

    def _store(self, sums, _):
        S, r = self._store_gated(sums), self.results
        with np.errstate(divide="ignore", invalid="ignore"):
            r.msd_axes = np.where(r.count[:, None] > 0, S / r.count[:, None], np.nan)
        r.msd = r.msd_axes.sum(axis=1)
