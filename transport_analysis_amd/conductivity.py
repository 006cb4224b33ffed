"""Einstein-Helfand ionic conductivity on MI355X, from positions.

The transport-analysis reference has no conductivity class; this one follows its ``ViscosityHelfand`` in
shape (constructor, ``run()``, a lag-index fit window).  Conductivity is a collective quantity: it is the
mean squared displacement of ONE sum over all atoms, the translational dipole

    M(t) = sum_n q_n (x_n(t) - x_n(0))

and not a mean of per-particle series.  The pass over the position slab that forms M (and, for the
Nernst-Einstein estimate, the weighted slab q (x - x[0])) runs in hand-written HIP (``k_cond_moment``
behind ``ta_conductivity`` of ``include/ta_hip.h``); both MSDs run on the library's Einstein MSD paths.
Positions only, like ``EinsteinMSD``: XTC / DCD trajectories qualify.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from ._base import CollectiveAnalysis

#: CODATA 2018 (exact SI values): elementary charge (C) and Boltzmann constant (J/K)
ELEMENTARY_CHARGE = 1.602176634e-19
BOLTZMANN_J_PER_K = 1.380649e-23


class ConductivityHelfand(CollectiveAnalysis):
    r"""Ionic conductivity by the Einstein-Helfand relation.

    .. math:: \Phi(k) = \frac{1}{T - k} \sum_{i < T - k} \sum_d (M_{i+k, d} - M_{i, d})^2, \qquad
              M_{t, d} = \sum_n q_n (x_{t, n, d} - x_{0, n, d})

    summed over the dimensions of ``dim_type``; :math:`\sigma` = slope of :math:`\Phi` against lag time
    / (2 D k_B <V> T_avg), with D the number of those dimensions.  In units:

        sigma [S/m] = e^2 10^22 / k_B[J/K] * slope[e^2 A^2 / ps] / (2 D <V>[A^3] T_avg[K])

    with CODATA e and k_B (e^2 A^2 / ps = e^2 10^-8 C^2 m^2 / s and A^3 = 10^-30 m^3).

    Parameters
    ----------
    atomgroup : AtomGroup — positions must be unwrapped for a meaningful moment: pass ``unwrap=True`` for a
        trajectory written wrapped into the box, or unwrap beforehand (MDAnalysis' ``NoJump``).
    temp_avg : float — average temperature (K), default 300.
    dim_type : {'xyz', 'xy', 'yz', 'xz', 'x', 'y', 'z'}
    linear_fit_window : (int, int) or None — lag indices [lo, hi) of the slope fit.  The fit is against
        lag time k * dt (ps; dt = the spacing of the analysed frames' times), not lag index.
    fft : bool — ``True``: the Einstein MSD's FFT form for both MSDs (up to 64 frames the exact direct
        kernel); ``False``: the direct forms.
    charges : array, keyword-only — one charge (e) per atom of ``atomgroup``; default ``atomgroup.charges``
        (a topology without charges raises MDAnalysis' missing-attribute error).
    nernst_einstein : bool, keyword-only, default False — also compute the self term
        sum_n q_n^2 MSD_n(k) (``results.timeseries_self``) and its conductivity: the Nernst-Einstein
        estimate, whose ratio to ``results.conductivity`` is the Haven ratio.  Costs one more
        slab-sized scratch on the device and an Einstein MSD lag-sum evaluation.
    unwrap : bool, keyword-only, default False — ``True``: undo the periodic wrapping of the staged positions on
        the device before the moment is formed, as MDAnalysis' ``NoJump`` does (see ``EinsteinMSD``: one
        crossing of the box would otherwise add q L to M).  Every analysed frame needs a box with lengths > 0, a
        non-orthogonal box needs ``dim_type='xyz'`` (else ``ValueError``), non-consecutive analysed frames give a
        ``UserWarning``; a particle that moves more than half a box between two analysed frames is not unwrapped
        correctly (not detected).  Under ``distributed=True`` every rank unwraps its own atoms.
    device, devices, distributed, stage_dtype : keyword-only — as for ``EinsteinMSD``.  Under
        ``distributed=True`` every rank forms the moment and self term of its block of atoms; the moments
        are summed over ranks BEFORE the collective MSD (the MSD of a sum is not the sum of the MSDs).

    Attributes
    ----------
    results.moment : (n_frames, D) float64 — M (e A).
    results.timeseries : (n_frames,) float64 — Phi (e^2 A^2), lag 0 exactly 0.
    results.timeseries_self : (n_frames,) float64 or None — sum_n q_n^2 MSD_n (e^2 A^2).
    results.conductivity, results.conductivity_self : S/m (only with ``linear_fit_window``).
    """

    _no_data_message = ("Helfand conductivity computation requires "
                        "positions and box volume in the trajectory")
    _updating_message = "UpdatingAtomGroups are not valid for conductivity computation"
    _by_particle_message = ("ConductivityHelfand has no per-particle result: conductivity is collective "
                            "(by_particle=True is not supported)")

    def __init__(self, atomgroup, temp_avg=300.0, dim_type="xyz", linear_fit_window=None, fft=True, *,
                 charges=None, nernst_einstein=False, unwrap=False, **kwargs):
        super().__init__(atomgroup, temp_avg, dim_type, linear_fit_window, fft, unwrap, kwargs)
        self.nernst_einstein = bool(nernst_einstein)
        self.charges = self._per_atom(atomgroup.charges if charges is None else charges, "charges", "values")

    def _prepare(self):
        super()._prepare()
        for key in ("conductivity", "conductivity_self"):  # a fit of an earlier run
            self.results.pop(key, None)
        self.results.moment = self.results.timeseries = self.results.timeseries_self = None

    def _moments(self, fft, lo, hi, correlate):
        moment, phi, self_ls = self._ctx.conductivity(fft, self.charges[lo:hi], self_term=self.nernst_einstein,
                                                      collective=correlate)
        return (moment, self_ls), phi

    def _no_moments(self):
        return np.zeros((self.n_frames, self.dim_fac)), (np.zeros(self.n_frames) if self.nernst_einstein else None)

    def _correlate(self, fft, sums):
        return self._ctx.moment_msd(sums[0], fft)

    def _store(self, sums, phi):
        self.results.moment, self.results.timeseries_self = sums
        self.results.timeseries = phi
        if self.linear_fit_window is not None:
            self.results.conductivity = self._sigma(phi)
            if self.nernst_einstein:
                self.results.conductivity_self = self._sigma(sums[1])

    def _sigma(self, series):
        return (ELEMENTARY_CHARGE ** 2 * 1e22 / BOLTZMANN_J_PER_K * self._slope(series)
                / (2 * self.dim_fac * self._vol_avg * self.temp_avg))
