"""Partial intermediate scattering functions F_ab(k, t) and partial structure factors S_ab(k) on MI355X, from positions.

    rho_a(k, t) = sum_{n in species a} w_n exp(i k . x_n(t))
    F_ab(k, t)  = 1/N < 1/2 (rho_a(k, t0)* rho_b(k, t0 + t) + rho_b(k, t0)* rho_a(k, t0 + t)) >,      S_ab(k) = F_ab(k, 0)

averaged over time origins t0, N all particles of the group (the Faber-Ziman-free convention of Kob and Andersen: the
partials add up to ``IntermediateScattering``'s F).  ONE pass over the position slab per chunk of wavevectors
(``k_species_density`` behind ``ta_partial_density`` of ``include/ta_hip.h``, hand-written HIP; a float32 slab is read as
float32, never widened first) reduces over the atoms in registers and leaves the densities of ALL species; their cross
term runs on the library's VACF paths by polarisation, for all wavevectors at once.  The Ashcroft-Langreth and
Bhatia-Thornton functions and neutron- or X-ray-weighted totals are host arithmetic on the partials.  There is no CPU
fallback.
"""
from __future__ import annotations

import numpy as np

from ._base import CollectiveAnalysis
from .onsager import index_species
from .scattering import BoxWavevectors


class PartialScattering(BoxWavevectors, CollectiveAnalysis):
    r"""Species-resolved collective intermediate scattering functions of a group of atoms (or of molecules' centres).

    .. math:: \rho_a(\mathbf{k}, t) = \sum_{n \in a} w_n e^{i \mathbf{k} \cdot \mathbf{x}_n(t)}, \qquad
              F_{ab}(\mathbf{k}, \tau) = \frac{1}{N} \frac{1}{T - \tau} \sum_{t < T - \tau} \frac{1}{2} \mathrm{Re}
              \left( \rho_a(t)^* \rho_b(t + \tau) + \rho_b(t)^* \rho_a(t + \tau) \right)

    Parameters
    ----------
    atomgroup : AtomGroup — the trajectory must hold positions.
    kvectors : (K, D) array in rad/A, used as they are (one component per dimension of ``dim_type``), or None.
    species : keyword-only — one label per atom of ``atomgroup`` (any sortable values, in any order; ``np.unique`` order
        defines the species index), or the name of a per-atom attribute of the group (``"types"``, ``"resnames"``).  At most
        8 distinct labels.  As for ``OnsagerHelfand``.
    weights : keyword-only — one weight per atom, or None (all 1: number densities; scattering lengths and charges per
        SPECIES enter afterwards through ``total(b)`` and ``bhatia_thornton(z)``).
    q, dq, max_vectors : keyword-only — instead of ``kvectors``: magnitudes (a scalar or a sequence, rad/A) and the shell
        width; the vectors are ``kvectors_from_box`` of the first analysed frame's box, at most ``max_vectors`` per shell.
        Exactly one of ``kvectors`` and ``q`` must be given.
    dim_type : {'xyz', 'xy', 'yz', 'xz', 'x', 'y', 'z'}
    fft : bool — ``True``: ``VelocityAutocorr``'s FFT evaluation for the correlations; ``False``: the direct forms.  The
        error of ``F_ab`` is relative to ``max(F_aa(0), F_bb(0))``, not to ``|F_ab|``.
    unwrap : bool, default False — undo periodic wrapping first.  Wavevectors commensurate with a constant box (``q=``) give
        phases that are invariant under wrapping: wrapped positions need no unwrapping.
    compound, compound_weights, reference_frame : keyword-only — as for ``IntermediateScattering``: the functions of
        molecules' centres; ``species`` is then one label per compound, or one per atom that is the same within every
        compound, ``weights`` one value per compound, and N the number of compounds.
    device, devices, distributed, stage_dtype : keyword-only — as for the other classes.  float32 staging stays float32 on
        the device (unless ``unwrap=True``, which works on float64 slabs).  Under ``distributed=True`` and ``devices=[...]``
        the densities of the blocks of atoms are summed BEFORE the correlation.
    A box is not needed with explicit ``kvectors``.  ``by_particle=True`` raises ``TypeError``.

    Attributes
    ----------
    results.species : the distinct labels, in species-index order; results.species_counts (S,) their particles.
    results.kvectors (K, D); results.shell (K,) the shell of every vector (explicit ``kvectors``: each its own);
    results.q_shell (n_shells,) the mean \|k\| per shell.
    results.density : (K, S, n_frames, 2) = (Re, Im) rho_a(k, t).
    results.f_partial_by_kvector : (n_frames, K, S, S); results.f_partial : (n_frames, n_shells, S, S) the shell mean;
    results.s_partial : (n_shells, S, S) = f_partial[0].  With unit weights the sum over a and b is
    ``IntermediateScattering``'s ``f``.
    """

    _accepts_compound = True
    _record_volumes = False
    _no_data_message = "Partial scattering function computation requires positions in the trajectory"
    _updating_message = "UpdatingAtomGroups are not valid for partial scattering function computation"
    _by_particle_message = ("PartialScattering has no per-particle result: the functions are sums over all atoms "
                            "(by_particle=True is not supported)")

    def __init__(self, atomgroup, kvectors=None, *, species, weights=None, q=None, dq=None, max_vectors=32, dim_type="xyz",
                 fft=True, unwrap=False, **kwargs):
        super().__init__(atomgroup, None, dim_type, None, fft, unwrap, kwargs)
        self._init_kvectors(kvectors, q, dq, max_vectors)
        if self.kvectors is not None:
            self.shell = np.arange(self.kvectors.shape[0])
        self.species, self.species_index = index_species(self._species_labels(species))
        self.n_species = max(int(self.species.size), 1)
        self.weights = None if weights is None else self._per_atom(weights, "weights", "values")

    def _set_options(self, dtype):
        # float32 staging stays float32 on the device: k_species_density reads it as it is (the unwrap pass works on float64
        # slabs)
        self._ctx.set_option("stage_device_f32", int(dtype == np.float32 and not self._unwrap))

    @staticmethod
    def _has_data(ts):
        return ts.has_positions

    def _prepare(self):
        super()._prepare()
        for key in ("kvectors", "shell", "q_shell", "density", "f_partial_by_kvector", "f_partial", "s_partial"):
            setattr(self.results, key, None)
        self.results.species = self.species
        self.results.species_counts = np.bincount(self.species_index, minlength=self.n_species).astype(np.int64)

    def _single_frame(self):
        self._box_kvectors()
        super()._single_frame()

    def _moments(self, fft, lo, hi, correlate):
        w = None if self.weights is None else self.weights[lo:hi]
        rho, cross = self._ctx.partial_density(fft, self.kvectors, self.species_index[lo:hi], self.n_species, w, cross=correlate)
        return (rho,), cross

    def _no_moments(self):
        return (np.zeros((self.kvectors.shape[0], self.n_species, self.n_frames, 2)),)

    def _correlate(self, fft, sums):
        return self._ctx.partial_cross(sums[0], fft)

    def _store(self, sums, cross):
        N = float(self.n_particles)
        r = self.results
        r.kvectors, r.shell = self.kvectors, self.shell
        norms = np.linalg.norm(self.kvectors, axis=1)
        n_shells = int(self.shell.max()) + 1
        counts = np.bincount(self.shell, minlength=n_shells)
        r.q_shell = np.bincount(self.shell, weights=norms) / counts
        r.density = sums[0]
        r.f_partial_by_kvector = np.ascontiguousarray(np.transpose(cross, (1, 0, 2, 3))) / N  # (K, T, S, S) -> (T, K, S, S)
        f = np.zeros((self.n_frames, n_shells, self.n_species, self.n_species))
        np.add.at(f, (slice(None), self.shell), r.f_partial_by_kvector)
        r.f_partial = f / counts[None, :, None, None]
        r.s_partial = r.f_partial[0].copy()

    def _partials(self, what):
        if self.results.get("f_partial") is None:
            raise RuntimeError(f"Analysis must be run prior to reading {what}")
        return self.results.f_partial

    def _per_species(self, values, name):
        a = np.asarray(values, dtype=np.float64).ravel()
        if a.size != self.n_species:
            raise ValueError(f"{name}: {a.size} values for {self.n_species} species")
        return a

    def total(self, b=None):
        """(n_frames, n_shells): ``sum_ab b_a b_b f_partial`` for one scattering length (or charge) per species in
        ``results.species`` order; ``b=None``: all ones, with unit weights ``IntermediateScattering``'s ``f``.  Nothing is
        normalised by ``<b^2>`` or ``<b>^2``: the conventions differ, the sum does not."""
        f = self._partials("total()")
        b = np.ones(self.n_species) if b is None else self._per_species(b, "b")
        return np.einsum("a,b,tsab->ts", b, b, f)

    def ashcroft_langreth(self):
        """(n_frames, n_shells, S, S): ``f_partial N / sqrt(N_a N_b)``, the Ashcroft-Langreth normalisation (``S_aa -> 1`` at
        large k with unit weights); NaN in the row and column of a species without particles."""
        f = self._partials("ashcroft_langreth()")
        n = self.results.species_counts.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return f * (float(self.n_particles) / np.sqrt(n[:, None] * n[None, :]))

    def bhatia_thornton(self, z=None):
        """Two species only (else ``ValueError``).  A dict of (n_frames, n_shells) arrays from the concentrations
        ``c_a = N_a / N``: ``nn = F_00 + F_11 + 2 F_01`` (number-number), ``nc = c_1 (F_00 + F_01) - c_0 (F_11 + F_01)``
        (number-concentration), ``cc = c_1^2 F_00 + c_0^2 F_11 - 2 c_0 c_1 F_01`` (concentration-concentration).  With ``z``
        (one charge number per species) also ``zz = sum_ab z_a z_b F_ab``, the charge-charge function whose k -> 0 limit
        is the Onsager conductivity's static counterpart."""
        f = self._partials("bhatia_thornton()")
        if self.n_species != 2:
            raise ValueError(f"bhatia_thornton: defined for two species, this analysis has {self.n_species}")
        c = self.results.species_counts / float(self.n_particles)
        f00, f11, f01 = f[..., 0, 0], f[..., 1, 1], f[..., 0, 1]
        out = {"nn": f00 + f11 + 2.0 * f01,
               "nc": c[1] * (f00 + f01) - c[0] * (f11 + f01),
               "cc": c[1] ** 2 * f00 + c[0] ** 2 * f11 - 2.0 * c[0] * c[1] * f01}
        if z is not None:
            z = self._per_species(z, "z")
            out["zz"] = np.einsum("a,b,tsab->ts", z, z, f)
        return out
