"""Species-resolved Onsager transport coefficients on MI355X, from positions.

``ConductivityHelfand`` gives the conductivity of the whole charge-weighted moment; this class resolves it by
species (Fong, Bergstrom, McCloskey, Persson, *Macromolecules* 2020 / *AIChE J.* 2020):

    L_ij = 1 / (2 D k_B T V) d/dt < dM_i(t) . dM_j(t) >,      M_s(t) = sum_{n in species s} w_n (x_n(t) - x_n(0))
    sigma = e^2 sum_ij z_i z_j L_ij,        t_i = z_i sum_j z_j L_ij / sum_kl z_k z_l L_kl

One pass over the position slab forms the moments of ALL species (``k_species_moment`` behind ``ta_onsager`` of
``include/ta_hip.h``, hand-written HIP); the cross mean squared displacements of the moments run on the library's
Einstein MSD paths by polarisation.  Positions only, like ``EinsteinMSD``.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._base import CollectiveAnalysis
from .conductivity import BOLTZMANN_J_PER_K, ELEMENTARY_CHARGE

#: ta_hip.h: TA_ONSAGER_MAX_SPECIES
MAX_SPECIES = 8


class SelfTerms:
    """What ``OnsagerHelfand`` and ``OnsagerGreenKubo`` share for ``self_terms=True``: the per-species self part
    ``sum_{n in s} w_n^2 f_n`` (``ta_species_self``: one sorted pass over the slab, then one lag-sum call per species) as
    a second array that adds up over atoms, beside the moments or currents."""

    _self_quantity = None  # _lib.SELF_MSD or _lib.SELF_VACF

    def _self_sums(self, fft, lo, hi):
        """(S, n_frames) of the atoms [lo, hi)"""
        w = None if self.weights is None else self.weights[lo:hi]
        return self._ctx.species_self(self._self_quantity, fft, self.species_index[lo:hi], self.n_species, w)[0]

    def _clear_self(self):
        for key in ("timeseries_self", "species_counts", "species_weight2", "onsager_self", "onsager_distinct"):
            self.results.pop(key, None)

    def _store_self(self, self_sums):
        """results.timeseries_self (n_frames, S), species_counts and species_weight2 = sum w^2 per species, of ALL atoms"""
        S = self.n_species
        w2 = np.ones(self.n_particles) if self.weights is None else self.weights ** 2
        self.results.timeseries_self = np.ascontiguousarray(self_sums.T)
        self.results.species_counts = np.bincount(self.species_index, minlength=S).astype(np.int64)
        self.results.species_weight2 = np.bincount(self.species_index, weights=w2, minlength=S)

    def _need_self(self, what):
        if not self.self_terms:
            raise ValueError(f"{what} needs the per-species self terms: pass self_terms=True")

    def _per_species(self, z):
        z = np.asarray(z, dtype=np.float64).ravel()
        if z.size != self.n_species:
            raise ValueError(f"z: {z.size} charges for {self.n_species} species")
        return z


def index_species(labels):
    """(the distinct labels in ``np.unique`` order, one int32 species index per atom); more than MAX_SPECIES distinct
    labels raise ValueError"""
    species, index = np.unique(labels, return_inverse=True)
    if species.size > MAX_SPECIES:
        raise ValueError(f"species: {species.size} distinct labels, at most {MAX_SPECIES} are supported")
    return species, np.ascontiguousarray(index, dtype=np.int32).ravel()


class OnsagerHelfand(SelfTerms, CollectiveAnalysis):
    r"""Onsager transport coefficients of the species of a system by the Einstein-Helfand relation.

    .. math:: C_{ij}(k) = \frac{1}{T - k} \sum_{t < T - k} \sum_d (M_{i; t+k, d} - M_{i; t, d}) (M_{j; t+k, d} - M_{j; t, d}),
              \qquad M_{s; t, d} = \sum_{n \in s} w_n (x_{t, n, d} - x_{0, n, d})

    summed over the dimensions of ``dim_type``; :math:`L_{ij}` = slope of :math:`C_{ij}` against lag time
    / (2 D k_B <V> T_avg), with D the number of those dimensions.

    Parameters
    ----------
    atomgroup : AtomGroup — positions must be unwrapped (``unwrap=True`` for a trajectory written wrapped into the box).
    species : one label per atom of ``atomgroup`` (any sortable values, in any order: interleaved topologies are
        fine; ``np.unique`` order defines the species index), or the name of a per-atom attribute of the group as a
        string (``"types"``, ``"resnames"``).  At most 8 distinct labels.
    temp_avg : float — average temperature (K), default 300.
    dim_type : {'xyz', 'xy', 'yz', 'xz', 'x', 'y', 'z'}
    linear_fit_window : (int, int) or None — lag indices [lo, hi) of the slope fits, against lag time k * dt (ps).
    fft : bool — ``True``: the Einstein MSD's FFT form for the cross MSDs (up to 64 frames the exact direct kernel);
        ``False``: the direct forms.  The error of ``C_ij`` is relative to ``max(C_ii, C_jj)``, not to ``|C_ij|``.
    weights : array, keyword-only — one weight per atom (default 1: ``M_s`` is the species' summed displacement, and
        charges enter through ``conductivity(z)``).  With ``weights=charges`` and one species, ``moments[0]`` and
        ``timeseries[:, 0, 0]`` are ``ConductivityHelfand``'s moment and Phi.
    unwrap : bool, keyword-only, default False — as for ``ConductivityHelfand``.
    self_terms : bool, keyword-only, default False — also compute the self part of every species,
        ``sum_{n in s} w_n^2 MSD_n(k)``, in one more pass over the slab (``k_species_sort`` behind ``ta_species_self``)
        and one MSD lag-sum call per species.
    compound, compound_weights, reference_frame : keyword-only — as for ``EinsteinMSD``: the moments and self terms of
        the centres (of mass) of molecules or ions instead of atoms, in the laboratory or the barycentric frame -- the
        quantities the papers above define.  With ``compound``, ``species`` is one label per compound, or one per atom
        that is the same within every compound (``species="resnames"``; else ``ValueError``), and ``weights`` one value
        per compound; ``results.compound_ids`` holds the compounds' labels, ``results.species_counts`` counts compounds.
    device, devices, distributed, stage_dtype : keyword-only — as for ``EinsteinMSD``.  Under ``distributed=True``
        every rank forms the moments of its block of atoms with its slice of the labels; the moments are summed over
        ranks BEFORE the correlation.

    Attributes
    ----------
    results.species : the distinct labels, in species-index order.
    results.moments : (S, n_frames, D) float64 — M (A times weight).
    results.timeseries : (n_frames, S, S) float64 — C (A^2 times weight^2), symmetric, lag 0 exactly 0.
    results.onsager : (S, S) float64, only with ``linear_fit_window`` — L_ij = slope x 1e22 / (2 D k_B <V> T_avg) in
        (J m s)^-1 per particle^2 (A^2 / ps = 1e-8 m^2 / s, A^3 = 1e-30 m^3); divide by N_A^2 for mol^2 J^-1 m^-1 s^-1.

    With ``self_terms=True``:
    results.timeseries_self : (n_frames, S) float64 — sum_{n in s} w_n^2 MSD_n (A^2 times weight^2), lag 0 exactly 0.
    results.species_counts, results.species_weight2 : (S,) — the atoms and sum w_n^2 of every species.
    results.onsager_self : (S,) float64, only with ``linear_fit_window`` — L_ii^self, slope x the factor of ``onsager``.
    results.onsager_distinct : (S, S) — ``onsager - diag(onsager_self)``.
    ``self_diffusivities()``, ``conductivity_nernst_einstein(z)`` and ``ionicity(z)`` read them.

    The Green-Kubo (velocity) form is ``OnsagerGreenKubo``.
    """

    _self_quantity = _lib.SELF_MSD
    _accepts_compound = True

    _no_data_message = ("Onsager coefficient computation requires "
                        "positions and box volume in the trajectory")
    _updating_message = "UpdatingAtomGroups are not valid for Onsager coefficient computation"
    _by_particle_message = ("OnsagerHelfand has no per-particle result: the Onsager coefficients are collective "
                            "(by_particle=True is not supported)")

    def __init__(self, atomgroup, species, temp_avg=300.0, dim_type="xyz", linear_fit_window=None, fft=True, *,
                 weights=None, unwrap=False, self_terms=False, **kwargs):
        super().__init__(atomgroup, temp_avg, dim_type, linear_fit_window, fft, unwrap, kwargs)
        self.self_terms = bool(self_terms)
        self.species, self.species_index = index_species(self._species_labels(species))
        self.n_species = max(int(self.species.size), 1)
        self.weights = None if weights is None else self._per_atom(weights, "weights", "values")

    def _prepare(self):
        super()._prepare()
        self.results.pop("onsager", None)  # a fit of an earlier run
        self._clear_self()
        self.results.species = self.species
        self.results.moments = self.results.timeseries = None

    def _moments(self, fft, lo, hi, correlate):
        w = None if self.weights is None else self.weights[lo:hi]
        moments, cross = self._ctx.onsager(fft, self.species_index[lo:hi], self.n_species, w, cross=correlate)
        if self.self_terms:
            return (moments, self._self_sums(fft, lo, hi)), cross
        return (moments,), cross

    def _no_moments(self):
        moments = np.zeros((self.n_species, self.n_frames, self.dim_fac))
        return (moments, np.zeros((self.n_species, self.n_frames))) if self.self_terms else (moments,)

    def _correlate(self, fft, sums):
        return self._ctx.onsager_cross(sums[0], fft)

    def _store(self, sums, cross):
        self.results.moments = sums[0]
        self.results.timeseries = cross
        if self.self_terms:
            self._store_self(sums[1])
        if self.linear_fit_window is not None:
            S = self.n_species
            factor = 1e22 / (2 * self.dim_fac * BOLTZMANN_J_PER_K * self._vol_avg * self.temp_avg)
            slopes = np.array([[self._slope(cross[:, i, j]) for j in range(S)] for i in range(S)])
            self.results.onsager = slopes * factor
            if self.self_terms:
                self.results.onsager_self = np.array([self._slope(sums[1][s]) for s in range(S)]) * factor
                self.results.onsager_distinct = self.results.onsager - np.diag(self.results.onsager_self)

    def _charge_weighted(self, z):
        if "onsager" not in self.results:
            raise ValueError("the Onsager coefficients need a fit: pass linear_fit_window=(lo, hi)")
        z = np.asarray(z, dtype=np.float64).ravel()
        if z.size != self.n_species:
            raise ValueError(f"z: {z.size} charges for {self.n_species} species")
        return z[:, None] * z[None, :] * self.results.onsager

    def conductivity(self, z):
        """sigma = e^2 sum_ij z_i z_j L_ij in S/m for one charge number per species (index order of
        ``results.species``); with unit weights this is ``ConductivityHelfand``'s value for charges ``z[species]``."""
        return ELEMENTARY_CHARGE ** 2 * float(self._charge_weighted(z).sum())

    def transference_numbers(self, z):
        """t_i = z_i sum_j z_j L_ij / sum_kl z_k z_l L_kl, one per species; they add up to 1."""
        zlz = self._charge_weighted(z)
        return zlz.sum(axis=1) / zlz.sum()

    def _fitted_self(self, what):
        self._need_self(what)
        if "onsager_self" not in self.results:
            raise ValueError("the self terms need a fit: pass linear_fit_window=(lo, hi)")
        return self.results.onsager_self

    def self_diffusivities(self):
        """(S,) self-diffusion coefficients in A^2 / ps: the slope of ``timeseries_self`` / (2 D sum_{n in s} w_n^2) --
        with unit weights the ``EinsteinMSD`` slope / (2 D) of the species' atoms; NaN for a species without atoms."""
        self._fitted_self("self_diffusivities()")
        slopes = np.array([self._slope(self.results.timeseries_self[:, s]) for s in range(self.n_species)])
        with np.errstate(invalid="ignore", divide="ignore"):
            return slopes / (2 * self.dim_fac * self.results.species_weight2)

    def conductivity_nernst_einstein(self, z):
        """sigma_NE = e^2 sum_i z_i^2 L_ii^self in S/m for one charge number per species: with unit weights
        ``ConductivityHelfand(nernst_einstein=True).results.conductivity_self`` for charges ``z[species]``."""
        L = self._fitted_self("conductivity_nernst_einstein(z)")
        return ELEMENTARY_CHARGE ** 2 * float((self._per_species(z) ** 2 * L).sum())

    def ionicity(self, z):
        """sigma / sigma_NE: 1 for uncorrelated ions, below 1 where ion pairs move together."""
        return self.conductivity(z) / self.conductivity_nernst_einstein(z)
