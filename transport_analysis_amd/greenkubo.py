"""Green-Kubo ionic conductivity and Onsager transport coefficients on MI355X, from velocities.

``ConductivityHelfand`` and ``OnsagerHelfand`` take the Einstein-Helfand route from positions; these two classes take the
Green-Kubo route from a velocity trajectory (TRR, or anything ``VelocityAutocorr`` accepts):

    L_ij = 1 / (D k_B T V) int_0^inf < J_i(0) . J_j(t) > dt,      J_s(t) = sum_{n in species s} w_n v_n(t)
    sigma = e^2 sum_ij z_i z_j L_ij,        t_i = z_i sum_j z_j L_ij / sum_kl z_k z_l L_kl

One pass over the velocity slab forms the currents of ALL species (``k_species_current`` behind ``ta_current`` of
``include/ta_hip.h``, hand-written HIP; a float32 slab is read as float32, never widened first); the cross-correlations of
the currents run on the library's VACF paths by polarisation.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from ._base import CollectiveAnalysis, UpdatingAtomGroup
from .conductivity import BOLTZMANN_J_PER_K, ELEMENTARY_CHARGE
from . import _lib
from .onsager import SelfTerms, index_species


class OnsagerGreenKubo(SelfTerms, CollectiveAnalysis):
    r"""Onsager transport coefficients of the species of a system by the Green-Kubo relation.

    .. math:: C_{ij}(k) = \frac{1}{2} \frac{1}{T - k} \sum_{t < T - k} \sum_d (J_{i; t, d} J_{j; t+k, d} + J_{j; t, d} J_{i; t+k, d}),
              \qquad J_{s; t, d} = \sum_{n \in s} w_n v_{t, n, d}

    summed over the dimensions of ``dim_type``; :math:`L_{ij}` = time integral of :math:`C_{ij}` / (D k_B <V> T_avg),
    with D the number of those dimensions -- the quantity ``OnsagerHelfand.results.onsager`` estimates from a slope / 2.

    Parameters
    ----------
    atomgroup : AtomGroup — the trajectory must hold velocities and a box.
    species : one label per atom of ``atomgroup``, or the name of a per-atom attribute, as for ``OnsagerHelfand``.  At
        most 8 distinct labels.
    temp_avg : float — average temperature (K), default 300.
    dim_type : {'xyz', 'xy', 'yz', 'xz', 'x', 'y', 'z'}
    fft : bool — ``True``: ``VelocityAutocorr``'s FFT evaluation for the correlations; ``False``: the direct forms.  The
        error of ``C_ij`` is relative to ``max(C_ii(0), C_jj(0))``, not to ``|C_ij|``.
    weights : array, keyword-only — one weight per atom (default 1; charges enter through ``conductivity(z)``).
    self_terms : bool, keyword-only, default False — also compute the self part of every species,
        ``sum_{n in s} w_n^2 VACF_n(k)``, in one more pass over the slab (``k_species_sort`` behind ``ta_species_self``,
        a float32 slab read as it is) and one VACF lag-sum call per species.
    device, devices, distributed, stage_dtype : keyword-only — as for ``VelocityAutocorr``.  float32 staging stays float32
        on the device at every number of frames: the current pass reads it as it is.  Under ``distributed=True`` every
        rank forms the currents of its block of atoms; they are summed over ranks BEFORE the correlation.
    compound, compound_weights, reference_frame : keyword-only — as for ``OnsagerHelfand``: the currents and self terms
        of the centre-of-mass velocities of molecules or ions, in the laboratory or the barycentric frame (the staged
        velocities minus the mass-weighted mean velocity of the group).  ``species`` and ``weights`` are then per compound
        (``species`` may also be given per atom, the same within every compound).  A float32 slab is read as it is.
    ``unwrap`` is not accepted: velocities are not wrapped.

    Attributes
    ----------
    results.species : the distinct labels, in species-index order.
    results.currents : (S, n_frames, D) float64 — J (A / ps times weight).
    results.timeseries : (n_frames, S, S) float64 — C (A^2 / ps^2 times weight^2), symmetric, lag 0 = <J_i . J_j>.

    ``onsager_gk`` / ``onsager_gk_odd`` integrate over a window of lags with ``VelocityAutocorr``'s convention
    (``start=0, stop=0, step=1``; ``stop=0``: all lags).

    With ``self_terms=True``: ``results.timeseries_self`` (n_frames, S) = sum_{n in s} w_n^2 <v_n(0) . v_n(k dt)> (lag 0
    kept), ``results.species_counts`` and ``results.species_weight2`` (S,); ``onsager_self_gk`` / ``onsager_self_gk_odd``
    integrate it as ``onsager_gk`` does C; ``self_diffusivities``, ``conductivity_nernst_einstein(z)`` and
    ``ionicity(z)`` read them.

    Not here: more than 8 species.
    """

    _self_quantity = _lib.SELF_VACF
    _accepts_compound = True

    _stage_arrays = ("velocities",)
    _no_data_message = ("Green-Kubo Onsager coefficient computation requires "
                        "velocities and box volume in the trajectory")
    _updating_message = "UpdatingAtomGroups are not valid for Green-Kubo Onsager coefficient computation"
    _by_particle_message = ("OnsagerGreenKubo has no per-particle result: the Onsager coefficients are collective "
                            "(by_particle=True is not supported)")

    def __init__(self, atomgroup, species, temp_avg=300.0, dim_type="xyz", fft=True, *, weights=None, self_terms=False,
                 **kwargs):
        if "unwrap" in kwargs:
            raise TypeError(f"{type(self).__name__} reads velocities, which are not wrapped: unwrap is not accepted")
        super().__init__(atomgroup, temp_avg, dim_type, None, fft, False, kwargs)
        self.species, self.species_index = index_species(self._species_labels(species))
        self.n_species = max(int(self.species.size), 1)
        self.weights = None if weights is None else self._particle_weights(weights)
        self.self_terms = bool(self_terms)
        self._cross = self._self = None

    def _particle_weights(self, weights):
        return self._per_atom(weights, "weights", "values")

    def _set_options(self, dtype):
        # float32 staging stays float32 on the device, whatever the number of frames: k_species_current reads it as it is
        self._ctx.set_option("stage_device_f32", int(dtype == np.float32))

    @staticmethod
    def _has_data(ts):
        return ts.has_velocities and ts.volume != 0

    def _prepare(self):
        super()._prepare()
        self._cross = self._self = None
        self._clear_results()
        self._clear_self()

    def _clear_results(self):
        self.results.species = self.species
        self.results.currents = self.results.timeseries = None

    def _moments(self, fft, lo, hi, correlate):
        w = None if self.weights is None else self.weights[lo:hi]
        currents, cross = self._ctx.current(fft, self.species_index[lo:hi], self.n_species, w, cross=correlate)
        if self.self_terms:
            return (currents, self._self_sums(fft, lo, hi)), cross
        return (currents,), cross

    def _no_moments(self):
        currents = np.zeros((self.n_species, self.n_frames, self.dim_fac))
        return (currents, np.zeros((self.n_species, self.n_frames))) if self.self_terms else (currents,)

    def _correlate(self, fft, sums):
        return self._ctx.current_cross(sums[0], fft)

    def _store(self, sums, cross):
        self._currents = sums[0]
        self._cross = cross
        self._publish()
        if self.self_terms:
            self._self = sums[1]
            self._store_self(self._self)

    def _publish(self):
        self.results.currents = self._currents
        self.results.timeseries = self._cross

    # --------------------------------------------- post-processing (host)
    def _factor(self):
        """(A^2 / ps) -> (J m s)^-1: 1e22 / (D k_B <V> T_avg), as ``OnsagerHelfand`` (whose slope carries a further 1/2)"""
        return 1e22 / (self.dim_fac * BOLTZMANN_J_PER_K * self._vol_avg * self.temp_avg)

    def _window(self, start, stop, step):
        if self._cross is None:
            raise RuntimeError("Analysis must be run prior to integrating the current correlations")
        stop = self.n_frames if stop == 0 else stop
        sl = slice(start, stop, step)
        return self.lag_times()[sl], self._cross[sl]

    def onsager_gk(self, start=0, stop=0, step=1):
        """(S, S) L_ij = trapezoid integral of C_ij over the lags ``[start:stop:step]`` x 1e22 / (D k_B <V> T_avg), in
        (J m s)^-1 per particle^2: the units of ``OnsagerHelfand.results.onsager``."""
        t, y = self._window(start, stop, step)
        dt = np.diff(t)[:, None, None]
        return (0.5 * (y[1:] + y[:-1]) * dt).sum(axis=0) * self._factor()

    def onsager_gk_odd(self, start=0, stop=0, step=1):
        """As ``onsager_gk`` by Simpson's rule (``scipy.integrate.simpson``, as ``self_diffusivity_gk_odd``)."""
        from scipy import integrate

        t, y = self._window(start, stop, step)
        return integrate.simpson(y=y, x=t, axis=0) * self._factor()

    def _self_window(self, start, stop, step, what):
        self._need_self(what)
        if self._self is None:
            raise RuntimeError("Analysis must be run prior to integrating the self terms")
        stop = self.n_frames if stop == 0 else stop
        sl = slice(start, stop, step)
        return self.lag_times()[sl], self._self.T[sl]

    def onsager_self_gk(self, start=0, stop=0, step=1):
        """(S,) L_ii^self = trapezoid integral of ``timeseries_self`` over the lags ``[start:stop:step]`` x the factor of
        ``onsager_gk``."""
        t, y = self._self_window(start, stop, step, "onsager_self_gk()")
        return (0.5 * (y[1:] + y[:-1]) * np.diff(t)[:, None]).sum(axis=0) * self._factor()

    def onsager_self_gk_odd(self, start=0, stop=0, step=1):
        """As ``onsager_self_gk`` by Simpson's rule."""
        from scipy import integrate

        t, y = self._self_window(start, stop, step, "onsager_self_gk_odd()")
        return integrate.simpson(y=y, x=t, axis=0) * self._factor()

    def self_diffusivities(self, start=0, stop=0, step=1, odd=False):
        """(S,) self-diffusion coefficients in A^2 / ps: the integral of ``timeseries_self`` / (D sum_{n in s} w_n^2) --
        with unit weights ``VelocityAutocorr.self_diffusivity_gk`` of the species' atoms; NaN for a species without
        atoms."""
        self._need_self("self_diffusivities()")
        L = self.onsager_self_gk_odd(start, stop, step) if odd else self.onsager_self_gk(start, stop, step)
        with np.errstate(invalid="ignore", divide="ignore"):
            return L / self._factor() / (self.dim_fac * self.results.species_weight2)

    def conductivity_nernst_einstein(self, z, start=0, stop=0, step=1, odd=False):
        """sigma_NE = e^2 sum_i z_i^2 L_ii^self in S/m for one charge number per species."""
        self._need_self("conductivity_nernst_einstein(z)")
        L = self.onsager_self_gk_odd(start, stop, step) if odd else self.onsager_self_gk(start, stop, step)
        return ELEMENTARY_CHARGE ** 2 * float((self._per_species(z) ** 2 * L).sum())

    def ionicity(self, z, start=0, stop=0, step=1, odd=False):
        """sigma / sigma_NE over the same window and rule."""
        return (self.conductivity(z, start, stop, step, odd)
                / self.conductivity_nernst_einstein(z, start, stop, step, odd))

    def running_integral(self):
        """(n_frames, S, S): the cumulative trapezoid integral of C over lag time in the units of ``onsager_gk`` -- the
        plateau of its entries is what a window is chosen by."""
        t, y = self._window(0, 0, 1)
        out = np.zeros_like(y)
        np.cumsum(0.5 * (y[1:] + y[:-1]) * np.diff(t)[:, None, None], axis=0, out=out[1:])
        return out * self._factor()

    def _charge_weighted(self, z, odd, window):
        z = np.asarray(z, dtype=np.float64).ravel()
        if z.size != self.n_species:
            raise ValueError(f"z: {z.size} charges for {self.n_species} species")
        L = self.onsager_gk_odd(*window) if odd else self.onsager_gk(*window)
        return z[:, None] * z[None, :] * L

    def conductivity(self, z, start=0, stop=0, step=1, odd=False):
        """sigma = e^2 sum_ij z_i z_j L_ij in S/m for one charge number per species (index order of
        ``results.species``); with unit weights this is ``ConductivityGreenKubo``'s value for charges ``z[species]``."""
        return ELEMENTARY_CHARGE ** 2 * float(self._charge_weighted(z, odd, (start, stop, step)).sum())

    def transference_numbers(self, z, start=0, stop=0, step=1, odd=False):
        """t_i = z_i sum_j z_j L_ij / sum_kl z_k z_l L_kl, one per species; they add up to 1."""
        zlz = self._charge_weighted(z, odd, (start, stop, step))
        return zlz.sum(axis=1) / zlz.sum()


class ConductivityGreenKubo(OnsagerGreenKubo):
    r"""Ionic conductivity by the Green-Kubo relation: the one-species form of ``OnsagerGreenKubo`` with the charges as
    weights, through the same library call (the same bits as ``OnsagerGreenKubo`` with one label and ``weights=charges``).

    .. math:: \sigma = \frac{e^2}{D k_B <V> T_{avg}} \int <J(0) . J(t)> dt, \qquad J_{t, d} = \sum_n q_n v_{t, n, d}

    Parameters: ``atomgroup``, ``charges`` (one charge (e) per atom; default ``atomgroup.charges``), ``temp_avg``,
    ``dim_type``, ``fft``, ``self_terms`` (``results.timeseries_self`` (n_frames, 1) = sum_n q_n^2 VACF_n: the
    Nernst-Einstein part, ``conductivity_nernst_einstein([1])``) and the placement keywords, as for ``OnsagerGreenKubo``.
    ``compound``, ``compound_weights``, ``reference_frame`` as for ``OnsagerGreenKubo``: ``charges`` is then one charge per
    compound, or one per atom (the default, ``atomgroup.charges``), which are added up within every compound.

    Attributes
    ----------
    results.current : (n_frames, D) float64 — J (e A / ps).
    results.timeseries : (n_frames,) float64 — <J(0) . J(k dt)> (e^2 A^2 / ps^2), lag 0 included.
    """

    _no_data_message = ("Green-Kubo conductivity computation requires "
                        "velocities and box volume in the trajectory")
    _updating_message = "UpdatingAtomGroups are not valid for Green-Kubo conductivity computation"
    _by_particle_message = ("ConductivityGreenKubo has no per-particle result: conductivity is collective "
                            "(by_particle=True is not supported)")

    def __init__(self, atomgroup, charges=None, temp_avg=300.0, dim_type="xyz", fft=True, **kwargs):
        if isinstance(atomgroup, UpdatingAtomGroup):
            raise TypeError(self._updating_message)
        if "weights" in kwargs:
            raise TypeError("ConductivityGreenKubo takes charges, not weights")
        self._charges_per_atom = charges is None  # the group's own charges: certainly one per atom
        self._species_per_atom = True             # (the one species, given per atom below)
        q = atomgroup.charges if charges is None else charges
        super().__init__(atomgroup, np.zeros(len(atomgroup), dtype=np.int32), temp_avg, dim_type, fft, weights=q, **kwargs)
        self.charges = self.weights

    def _particle_weights(self, charges):
        q = np.asarray(charges, dtype=np.float64).ravel()
        if self._plan is None or self._compound is None:
            return super()._particle_weights(q)
        from .compound import same_order

        n, C = self._n_atoms, self.n_particles
        if q.size == n == C and not self._charges_per_atom and not same_order(self._compound_index, C):
            raise ValueError(f"charges: {q.size} values for {n} atoms in {C} one-atom compounds whose order (np.unique of the "
                             "labels) is not the atoms': per atom or per compound cannot be told apart; give the compound "
                             "labels in increasing order, or leave charges=None for the group's own")
        if q.size == n and (self._charges_per_atom or n != C):  # per atom: a compound's charge is their sum
            return np.bincount(self._compound_index, weights=q, minlength=C)
        return super()._particle_weights(q)

    def _clear_results(self):
        self.results.current = self.results.timeseries = None

    def _publish(self):
        self.results.current = self._currents[0]
        self.results.timeseries = self._cross[:, 0, 0]

    def conductivity_gk(self, start=0, stop=0, step=1):
        """sigma in S/m, trapezoid rule over the lags ``[start:stop:step]``."""
        return ELEMENTARY_CHARGE ** 2 * float(self.onsager_gk(start, stop, step)[0, 0])

    def conductivity_gk_odd(self, start=0, stop=0, step=1):
        """sigma in S/m, Simpson's rule."""
        return ELEMENTARY_CHARGE ** 2 * float(self.onsager_gk_odd(start, stop, step)[0, 0])
