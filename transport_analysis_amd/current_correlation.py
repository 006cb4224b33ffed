"""Longitudinal and transverse current correlation functions C_L(k, t) and C_T(k, t) on MI355X, from velocities and positions.

    j(k, t)   = sum_n w_n v_n(t) exp(i k . x_n(t))
    C_L(k, t) = 1/N < j_L(k, t0)* j_L(k, t0 + t) >,             j_L = k^ . j
    C_T(k, t) = 1/(D - 1) 1/N < j_T(k, t0)* . j_T(k, t0 + t) >,    j_T = j - k^ j_L

averaged over time origins t0.  One fused pass over BOTH staged slabs (``k_kcurrent`` behind ``ta_kcurrent`` of
``include/ta_hip.h``, hand-written HIP; float32 slabs are read as float32, never widened first) reduces over the atoms in
registers and leaves the current; its projections are autocorrelated on the library's VACF paths.  The peak of the
spectrum of C_L gives the sound dispersion, the decay of C_T the wavevector-dependent shear viscosity; with charges as
weights the functions are those of the charge current.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from ._base import CollectiveAnalysis
from .scattering import BoxWavevectors


class CurrentCorrelation(BoxWavevectors, CollectiveAnalysis):
    r"""Longitudinal and transverse current correlation functions of a group of atoms.

    .. math:: \mathbf{j}(\mathbf{k}, t) = \sum_n w_n \mathbf{v}_n(t) e^{i \mathbf{k} \cdot \mathbf{x}_n(t)}, \qquad
              C_L(\mathbf{k}, \tau) = \frac{1}{N} \frac{1}{T - \tau} \sum_{t < T - \tau} \mathrm{Re}\, j_L(t)^* j_L(t + \tau), \qquad
              C_T(\mathbf{k}, \tau) = \frac{1}{D - 1} \frac{1}{N} \frac{1}{T - \tau} \sum_{t < T - \tau} \mathrm{Re}\,
              \mathbf{j}_T(t)^* \cdot \mathbf{j}_T(t + \tau)

    Parameters
    ----------
    atomgroup : AtomGroup — the trajectory must hold velocities and positions.
    kvectors : (K, D) array in rad/A, used as they are (one component per dimension of ``dim_type``; none may be zero), or
        None.
    q, dq, max_vectors : instead of ``kvectors``: magnitudes (a scalar or a sequence, rad/A) and, keyword-only, the shell
        width; the vectors are ``kvectors_from_box`` of the first analysed frame's box, at most ``max_vectors`` per shell,
        as for ``IntermediateScattering``.  Exactly one of ``kvectors`` and ``q`` must be given.
    weights : keyword-only — ``"mass"`` (the default: the momentum current), ``"charge"`` (the charge current), ``None``
        (all 1: the particle current) or one value per atom.
    dim_type : {'xyz', 'xy', 'yz', 'xz', 'x', 'y', 'z'} — with one dimension there is no transverse part (zeros).
    fft : bool — ``True``: ``VelocityAutocorr``'s FFT evaluation for the correlations; ``False``: the direct forms.
    unwrap : bool, default False — undo periodic wrapping of the positions first.  Wavevectors commensurate with a constant
        box (``q=``) give phases that are invariant under wrapping: wrapped positions need no unwrapping.
    device, devices, distributed, stage_dtype : keyword-only — as for the other classes.  float32 staging stays float32 on
        the device (unless ``unwrap=True``, which works on float64 slabs).  Under ``distributed=True`` and
        ``devices=[...]`` the currents of the blocks of atoms are summed BEFORE the correlations.
    ``compound``, ``reference_frame`` and ``by_particle=True`` raise ``TypeError``: the reduction to molecules takes one
    staged slab, and the functions are sums over all atoms.

    Attributes
    ----------
    results.kvectors (K, D); results.k (K,) their magnitudes; results.times (n_frames,) the lag times (ps);
    results.current (K, n_frames, D, 2) = (Re, Im) j(k, t); results.cl, results.ct (n_frames, K); results.volume the mean
    box volume; with ``q=``: results.shell (K,), results.k_shell (n_shells,), results.cl_shell and results.ct_shell
    (n_frames, n_shells), the means over a shell's vectors.
    """

    _stage_arrays = ("velocities", "positions")
    _record_volumes = True
    _no_data_message = "Current correlation function computation requires velocities and positions in the trajectory"
    _updating_message = "UpdatingAtomGroups are not valid for current correlation function computation"
    _by_particle_message = ("CurrentCorrelation has no per-particle result: the functions are sums over all atoms "
                            "(by_particle=True is not supported)")

    def __init__(self, atomgroup, kvectors=None, q=None, *, dq=None, max_vectors=32, weights="mass", dim_type="xyz", fft=True,
                 unwrap=False, **kwargs):
        for key in ("compound", "compound_weights", "reference_frame"):
            if key in kwargs:
                raise TypeError(f"CurrentCorrelation does not take {key}: the reduction to molecules (ta_compound) takes one "
                                "staged slab, and the current needs velocities and positions")
        super().__init__(atomgroup, None, dim_type, None, fft, unwrap, kwargs)
        self._init_kvectors(kvectors, q, dq, max_vectors)
        if self.kvectors is not None:
            with np.errstate(over="ignore", under="ignore"):
                n2 = (self.kvectors * self.kvectors).sum(axis=1)  # (the library divides by its root)
            if not np.all(np.isfinite(n2)) or not np.all(n2 > 0.0):
                raise ValueError("kvectors: none may be zero, or too small or too large to normalise (k = 0 is "
                                 "ConductivityGreenKubo's current)")
        if isinstance(weights, str):
            if weights not in ("mass", "charge"):
                raise ValueError(f"weights: {weights!r}, expected 'mass', 'charge', None or one value per atom")
            attr = "masses" if weights == "mass" else "charges"
            self.weights = self._per_atom(self._group_attr(attr, f"weights={weights!r}"), "weights", "values")
        else:
            self.weights = None if weights is None else self._per_atom(weights, "weights", "values")

    def _set_options(self, dtype):
        # float32 staging stays float32 on the device: k_kcurrent reads both slabs as they are (the unwrap pass works on
        # float64 slabs)
        self._ctx.set_option("stage_device_f32", int(dtype == np.float32 and not self._unwrap))

    @staticmethod
    def _has_data(ts):
        return ts.has_velocities and ts.has_positions

    def _prepare(self):
        super()._prepare()
        for key in ("kvectors", "k", "times", "current", "cl", "ct", "volume", "shell", "k_shell", "cl_shell", "ct_shell"):
            setattr(self.results, key, None)

    def _single_frame(self):
        self._box_kvectors()
        super()._single_frame()

    def _moments(self, fft, lo, hi, correlate):
        w = None if self.weights is None else self.weights[lo:hi]
        cur, lon, tr = self._ctx.kcurrent(fft, self.kvectors, w, longitudinal=correlate, transverse=correlate)
        return (cur,), ((lon, tr) if correlate else None)

    def _no_moments(self):
        return (np.zeros((self.kvectors.shape[0], self.n_frames, self.dim_fac, 2)),)

    def _correlate(self, fft, sums):
        return self._ctx.kcurrent_correlate(sums[0], self.kvectors, fft)

    def _store(self, sums, corr):
        N = float(self.n_particles)
        r = self.results
        r.kvectors, r.k = self.kvectors, np.linalg.norm(self.kvectors, axis=1)
        r.times = self.lag_times()
        r.current = sums[0]
        r.cl = np.ascontiguousarray(corr[0].T) / N
        r.ct = np.ascontiguousarray(corr[1].T) / N
        r.volume = self._vol_avg
        if self.shell is not None:
            r.shell = self.shell
            r.k_shell = np.bincount(self.shell, weights=r.k) / np.bincount(self.shell)
            r.cl_shell, r.ct_shell = self._shell_mean(r.cl), self._shell_mean(r.ct)

    def spectrum(self, window="hann"):
        """(omega (n_frames,) in rad/ps, cl_w (n_frames, K), ct_w (n_frames, K)): the windowed cosine transform of the lag
        series, ``C(omega) = dt (w_0 C_0 + 2 sum_{tau >= 1} w_tau C_tau cos(omega tau dt))`` at ``omega_m = pi m / (n_frames
        dt)``, on the host.  ``window``: ``"hann"`` (``w_tau = (1 + cos(pi tau / n_frames)) / 2``: 1 at lag 0, 0 at the end)
        or ``None`` (all 1).  Nothing is fitted: the peak of ``cl_w`` along omega is the sound mode's frequency, the
        width of ``ct_w`` the shear relaxation rate."""
        if self.results.get("cl") is None:
            raise RuntimeError("Analysis must be run prior to reading the spectrum")
        if window not in ("hann", None):
            raise ValueError(f"window: {window!r}, expected 'hann' or None")
        T = self.n_frames
        dt = float(self.times[1] - self.times[0]) if T > 1 else 1.0
        tau = np.arange(T)
        w = 0.5 * (1.0 + np.cos(np.pi * tau / T)) if window == "hann" else np.ones(T)
        w = w * np.where(tau == 0, 1.0, 2.0) * dt
        omega = np.pi * np.arange(T) / (T * dt)
        out = [np.empty_like(self.results.cl), np.empty_like(self.results.ct)]
        for m0 in range(0, T, 256):  # (a block of frequencies at a time: the cosine table stays small)
            c = np.cos(np.outer(omega[m0:m0 + 256] * dt, tau)) * w
            out[0][m0:m0 + 256] = c @ self.results.cl
            out[1][m0:m0 + 256] = c @ self.results.ct
        return omega, out[0], out[1]
