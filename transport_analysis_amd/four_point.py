"""Four-point structure factor S_4(k, t) of the overlap field on MI355X, from positions.

    W(k, t0, tau)  = sum_n Theta(a - |x_n(t0 + tau) - x_n(t0)|) exp(i k . x_n(t0))     (the overlap field's density)
    S_4(k, tau)    = ( < |W|^2 > - | < W > |^2 ) / N                                    (the averages over time origins t0)

``DynamicSusceptibility`` gives chi_4(tau) = S_4(k -> 0, tau): how strong dynamic heterogeneity is.  How far it reaches -- the
dynamic correlation length xi_4(tau) -- is in the wavevector dependence of S_4 at small k.  Like chi_4 it is a variance over
origins, so the per-origin sums are what the library computes (``k_overlap_density`` behind ``ta_overlap_density`` of
``include/ta_hip.h``, hand-written HIP: the phase belongs to the origin frame, so one evaluation per atom, origin frame and
wavevector serves every lag and cutoff of a launch; a float32 slab is read as float32, never widened first) -- W adds up
over atoms, |W|^2 does not, so blocks of atoms on several devices or ranks are summed BEFORE anything is squared here, in
float64 on the host.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from ._base import CollectiveAnalysis
from .scattering import BoxWavevectors
from .susceptibility import _check_cutoffs
from .vanhove import _VanHove, _check_lags, log_lags


class FourPointStructureFactor(BoxWavevectors, CollectiveAnalysis):
    r"""Four-point structure factor of the self-overlap field of a group of atoms (or of molecules' centres).

    .. math:: W(\mathbf{k}, t_0, \tau) = \sum_n \Theta(a - |\mathbf{x}_n(t_0 + \tau) - \mathbf{x}_n(t_0)|)\,
              e^{i \mathbf{k} \cdot \mathbf{x}_n(t_0)}, \qquad
              S_4(\mathbf{k}, \tau) = \frac{\langle |W|^2 \rangle - |\langle W \rangle|^2}{N}

    with the averages over the :math:`T - \tau` time origins; :math:`S_4(\mathbf{k} \to 0, \tau) = \chi_4(\tau)` of
    ``DynamicSusceptibility`` (an explicit ``k = 0`` gives exactly that).  The comparison is strict: an atom exactly at
    distance a is not counted.

    Two things to keep in mind when reading ``s4``, as for ``chi4``.  It is ensemble-dependent: this is the fluctuation at
    the trajectory's fixed N (and whatever else the simulation holds fixed), which matters most at the smallest k.  And
    consecutive origins are correlated: the variance over all ``T - tau`` origins is the plain (``ddof=0``) one, not an
    estimate with ``T - tau`` independent samples; ``results.w_by_origin`` is there for block averages and strides of
    one's own.  No fit of a correlation length is offered: ``s4`` against ``q_shell`` is what such a fit starts from.

    Parameters
    ----------
    atomgroup : AtomGroup — the trajectory must hold positions.
    kvectors : (K, D) array in rad/A, used as they are (one component per dimension of ``dim_type``), or None.
    lags : integer frame lags, strictly increasing, below the number of analysed frames; ``None`` (the default):
        ``log_lags(n_frames, per_decade=8)``.
    cutoff : keyword-only — the overlap length a, a scalar or a strictly increasing sequence of up to 4 (one pass
        serves them all).
    q, dq, max_vectors : keyword-only — instead of ``kvectors``: magnitudes (a scalar or a sequence, rad/A) and the shell
        width; the vectors are ``kvectors_from_box`` of the first analysed frame's box, at most ``max_vectors`` per shell.
        Exactly one of ``kvectors`` and ``q`` must be given.
    dim_type : {'xyz', 'xy', 'yz', 'xz', 'x', 'y', 'z'}.
    unwrap : bool, default False — undo periodic wrapping first (``EinsteinMSD``'s).  The phase of a wavevector
        commensurate with a constant box (``q=``) is invariant under wrapping and needs none; the DISPLACEMENT behind the
        overlap does: wrapped positions give wrong displacements, so trajectories whose atoms cross the box need
        ``unwrap=True`` here even with box wavevectors.
    compound, compound_weights, reference_frame : keyword-only — as for ``DynamicSusceptibility``: the field of molecules'
        centres; N is then the number of compounds.
    device, devices, distributed, stage_dtype : keyword-only — as for the other classes.  float32 staging stays float32
        on the device (unless ``unwrap=True``, which works on float64 slabs).  Under ``distributed=True`` and
        ``devices=[...]`` the blocks' W are added before anything is squared.
    A box is needed only for ``q=`` and ``unwrap``.  ``by_particle=True`` raises ``TypeError``.

    Attributes
    ----------
    results.lags (L,); results.times (L,) ps; results.cutoffs (C,); results.n_origins (L,) = T - lags;
    results.kvectors (K, D); results.shell (K,) the shell of every vector (explicit ``kvectors``: each its own);
    results.q_shell (n_shells,) the mean \|k\| per shell; results.w_by_origin (K, C, L, T) complex128, the raw sums, zeros
    at t0 >= T - lag; results.s4_by_kvector (K, C, L) = (mean \|W\|^2 - \|mean W\|^2) / N over the valid origins (two-pass),
    NaN where there are fewer than two; results.s4_uncentred_by_kvector (K, C, L) = mean \|W\|^2 / N; results.s4 and
    results.s4_uncentred (n_shells, C, L), the shell means.  A scalar ``cutoff`` keeps the axis of length 1.
    """

    _accepts_compound = True
    _record_volumes = False
    _no_data_message = "Four-point structure factor computation requires positions in the trajectory"
    _updating_message = "UpdatingAtomGroups are not valid for four-point structure factor computation"
    _by_particle_message = ("FourPointStructureFactor has no per-particle result: the overlap field's density is a sum over "
                            "all atoms (by_particle=True is not supported)")
    _result_keys = ("lags", "times", "cutoffs", "kvectors", "shell", "q_shell", "n_origins", "w_by_origin", "s4_by_kvector",
                    "s4_uncentred_by_kvector", "s4", "s4_uncentred")

    def __init__(self, atomgroup, kvectors=None, lags=None, *, cutoff, q=None, dq=None, max_vectors=32, dim_type="xyz",
                 unwrap=False, **kwargs):
        super().__init__(atomgroup, None, dim_type, None, False, unwrap, kwargs)
        self._init_kvectors(kvectors, q, dq, max_vectors)
        if self.kvectors is not None:
            self.shell = np.arange(self.kvectors.shape[0])
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

    def _single_frame(self):
        self._box_kvectors()
        super()._single_frame()

    def _shape(self):
        return (self.kvectors.shape[0], self.cutoffs.size, self._lags.size, self.n_frames)

    def _moments(self, fft, lo, hi, correlate):
        # (the sums travel as float64 (..., 2): what adds up over members and ranks)
        w = self._ctx.overlap_density(self.kvectors, self._lags, self.cutoffs)
        return (np.ascontiguousarray(w).view(np.float64).reshape(self._shape() + (2,)),), None

    def _no_moments(self):
        return (np.zeros(self._shape() + (2,)),)

    def _correlate(self, fft, sums):
        return None  # the sums are the result: there is no correlation step

    def _store(self, sums, _):
        W = np.ascontiguousarray(sums[0], dtype=np.float64).view(np.complex128)[..., 0]
        r, T, N = self.results, self.n_frames, float(self.n_particles)
        r.lags = self._lags
        r.times = self._lags * (float(self.times[1] - self.times[0]) if T > 1 else 0.0)
        r.cutoffs = self.cutoffs
        r.kvectors, r.shell = self.kvectors, self.shell
        n_shells = int(self.shell.max()) + 1
        counts = np.bincount(self.shell, minlength=n_shells)
        r.q_shell = np.bincount(self.shell, weights=np.linalg.norm(self.kvectors, axis=1)) / counts
        r.n_origins = T - self._lags
        r.w_by_origin = W
        r.s4_by_kvector = np.full(W.shape[:3], np.nan)
        r.s4_uncentred_by_kvector = np.empty(W.shape[:3])
        for l, n in enumerate(r.n_origins):
            valid = W[:, :, l, :n]
            r.s4_uncentred_by_kvector[:, :, l] = (valid.real ** 2 + valid.imag ** 2).mean(axis=2) / N
            if n >= 2:
                dev = valid - valid.mean(axis=2, keepdims=True)  # (two-pass: the deviations from the mean, then their squares)
                r.s4_by_kvector[:, :, l] = (dev.real ** 2 + dev.imag ** 2).mean(axis=2) / N
        for key in ("s4", "s4_uncentred"):
            by_k = getattr(r, key + "_by_kvector")
            out = np.zeros((n_shells,) + by_k.shape[1:])
            np.add.at(out, self.shell, by_k)
            setattr(r, key, out / counts[:, None, None])
