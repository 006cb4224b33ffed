"""Rotational (orientational) correlation functions C_1(t), C_2(t) and the collective dipole sum on MI355X, from positions.

    C_l(tau) = 1/N 1/(T - tau) sum_{t < T - tau} sum_n P_l(u_n(t + tau) . u_n(t)),   l = 1, 2

for molecule-fixed unit vectors u_n(t): a bond a -> b, the bisector of a -> b and a -> c (a water molecule's dipole
direction with a = O) or the normal of the plane through a, b, c.  C_1 is what dielectric and infrared relaxation see, C_2
what NMR and fluorescence anisotropy do.  The collective partner is the autocorrelation of M(t) = sum_n w_n u_n(t), the
total dipole, with the Kirkwood factor G_K = <|M|^2> / sum_n w_n^2.

One pass over the position slab per rank (``k_orient`` behind ``ta_orient`` of ``include/ta_hip.h``, hand-written HIP; a
float32 slab is read as float32, never widened first) turns the gathered atoms into orientation columns: u itself for
l = 1 and the six independent columns of Q = u (x) u - 1/3 for l = 2, since P_2(u . u') = 3/2 Q : Q'.  The library's VACF
lag sums of those columns are the correlation functions, its species-sum pass the dipole.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._base import CollectiveAnalysis, first_crossing


def group_indices(atomgroup, universe_indices):
    """Universe atom indices (any integer array, e.g. ``ag.bonds.indices`` or ``ag.angles.indices`` of MDAnalysis) as
    positions within ``atomgroup`` -- what ``OrientationalCorrelation`` takes as ``vectors``.  An atom that is not in the
    group: ``ValueError``."""
    ix = getattr(atomgroup, "ix", None)
    if ix is None:
        ix = getattr(atomgroup, "indices")
    ix = np.asarray(ix, dtype=np.int64).ravel()
    want = np.asarray(universe_indices)
    if want.size and not np.issubdtype(want.dtype, np.integer):
        raise ValueError(f"universe_indices: dtype {want.dtype}, expected integers")
    want = want.astype(np.int64)
    order = np.argsort(ix, kind="stable")
    pos = np.searchsorted(ix[order], want.ravel())
    pos = np.minimum(pos, max(ix.size - 1, 0))
    found = ix[order][pos] == want.ravel() if ix.size else np.zeros(want.size, dtype=bool)
    if not np.all(found):
        missing = np.unique(want.ravel()[~found])
        raise ValueError(f"atoms {[int(i) for i in missing[:8]]}{' ...' if missing.size > 8 else ''} are not in the atom group")
    return order[pos].reshape(want.shape)


class OrientationalCorrelation(CollectiveAnalysis):
    r"""First- and second-rank rotational autocorrelation functions of molecule-fixed unit vectors, and their dipole sum.

    .. math:: C_l(\tau) = \frac{1}{N} \frac{1}{T - \tau} \sum_{t < T - \tau} \sum_n
              P_l(\mathbf{u}_n(t + \tau) \cdot \mathbf{u}_n(t)), \qquad
              \mathbf{M}(t) = \sum_n w_n \mathbf{u}_n(t), \qquad G_K = \frac{\langle |\mathbf{M}|^2 \rangle}{\sum_n w_n^2}

    Parameters
    ----------
    atomgroup : AtomGroup — the trajectory must hold positions.
    vectors : integer (N, 2) array for ``mode="bond"``, (N, 3) for the other modes — positions WITHIN the group
        (``group_indices`` maps universe indices such as ``ag.bonds.indices``).  The atoms of a row must differ.
    mode : {'bond', 'bisector', 'normal'} — (a, b): the direction a -> b; (a, b, c): the sum, or the cross product, of
        a -> b and a -> c.
    minimum_image : bool, default True — reduce every difference by one image step per axis with the frame's own box
        (orthorhombic and triclinic; constant or per frame): the minimum image while the vector is shorter than half the
        smallest box width, so molecules that the trajectory wraps across a face need no unwrapping.  Every frame then
        needs a box.  ``False``: the positions are used as they are.
    weights : (N,) values or None (all 1) — the dipole magnitudes w_n; they enter ``total``, ``total_acf`` and
        ``kirkwood`` only.
    fft : bool — ``True``: ``VelocityAutocorr``'s FFT evaluation for the correlations; ``False``: the direct forms.
    collective : bool, default True — also the autocorrelation of the total.
    device, stage_dtype : keyword-only — as for the other classes.  float32 staging stays float32 on the device: the
        orientation pass reads it as it is.  ``devices=[...]`` and ``distributed=True`` raise ``ValueError`` (the atoms
        would be split by index, and a vector's atoms would have to share a shard); ``by_particle=True`` raises
        ``TypeError``.

    Attributes
    ----------
    results.c1, results.c2 (n_frames,) — 1 at lag 0 for non-degenerate vectors; results.total (n_frames, 3) = M(t);
    results.total_acf (n_frames,) = <M(t) . M(t + tau)> (``collective``); results.kirkwood = mean_t |M|^2 / sum w^2.
    """

    _record_volumes = False
    _no_data_message = "Orientational correlation function computation requires positions in the trajectory"
    _updating_message = "UpdatingAtomGroups are not valid for orientational correlation function computation"
    _by_particle_message = ("OrientationalCorrelation has no per-particle result: the functions are sums over all vectors "
                            "(by_particle=True is not supported)")

    def __init__(self, atomgroup, vectors, *, mode="bond", minimum_image=True, weights=None, fft=True, collective=True, **kwargs):
        for key, what in (("devices", "devices=[...]"), ("distributed", "distributed=True")):
            if kwargs.get(key):
                raise ValueError(f"OrientationalCorrelation: {what} is not available -- the atoms are split over the GPUs by "
                                 "index, and all atoms of a molecule would have to share a shard")
        kwargs.pop("devices", None), kwargs.pop("distributed", None)
        super().__init__(atomgroup, None, "xyz", None, fft, False, kwargs)
        if mode not in _lib.ORIENT_MODES:
            raise ValueError(f"mode: {mode!r}, expected one of {sorted(_lib.ORIENT_MODES)}")
        self.mode = mode
        width = 2 if mode == "bond" else 3
        v = np.asarray(vectors)
        if v.ndim != 2 or v.shape[0] < 1 or v.shape[1] != width or not np.issubdtype(v.dtype, np.integer):
            raise ValueError(f"vectors: shape {v.shape} and dtype {v.dtype}, expected an integer (N, {width}) array of positions "
                             f"within the group for mode={mode!r}")
        if v.min() < 0 or v.max() >= self.n_particles:
            raise ValueError(f"vectors: entries must be positions within the group, 0 ... {self.n_particles - 1}")
        s = np.sort(v, axis=1)
        if np.any(s[:, 1:] == s[:, :-1]):
            raise ValueError(f"vectors: row {int(np.flatnonzero(np.any(s[:, 1:] == s[:, :-1], axis=1))[0])} names an atom twice")
        self.vectors = np.ascontiguousarray(v, dtype=np.int32)
        self.n_vectors = int(v.shape[0])
        self.minimum_image = bool(minimum_image)
        self.collective = bool(collective)
        self.weights = None
        if weights is not None:
            w = np.asarray(weights, dtype=np.float64).ravel()
            if w.size != self.n_vectors or not np.all(np.isfinite(w)):
                raise ValueError(f"weights: {w.size} values for {self.n_vectors} vectors (and all of them must be finite)")
            self.weights = w

    def _set_options(self, dtype):
        # float32 staging stays float32 on the device: k_orient reads it as it is
        self._ctx.set_option("stage_device_f32", int(dtype == np.float32))

    @staticmethod
    def _has_data(ts):
        return ts.has_positions

    def _prepare(self):
        super()._prepare()
        self._image_boxes = np.zeros((self.n_frames, 6)) if self.minimum_image else None
        for key in ("c1", "c2", "total", "total_acf", "kirkwood"):
            setattr(self.results, key, None)

    def _single_frame(self):
        if self._image_boxes is not None:
            try:
                self._image_boxes[self._frame_index] = self._unwrap_box(self._ts)
            except ValueError as err:  # (the checks of unwrap=True, under this class's keyword)
                raise ValueError(str(err).replace("unwrap=True", "minimum_image=True")) from None
        super()._single_frame()

    def _moments(self, fft, lo, hi, correlate):
        c1, c2, total, coll = self._ctx.orient(fft, self.vectors, self.mode, dimensions=self._image_boxes, weights=self.weights,
                                               collective=self.collective and correlate)
        return (c1, c2, total), coll

    def _store(self, sums, coll):
        N = float(self.n_vectors)
        r = self.results
        r.c1 = sums[0] / N
        r.c2 = 1.5 * sums[1] / N
        r.total = sums[2]
        r.total_acf = coll
        w2 = float(np.sum(self.weights ** 2)) if self.weights is not None else N
        r.kirkwood = float(np.mean(np.sum(r.total ** 2, axis=1)) / w2) if w2 > 0 else np.nan

    def relaxation_times(self, level=1.0 / np.e):
        """(tau_1, tau_2): the lag times (ps) at which ``c1 / c1[0]`` and ``c2 / c2[0]`` first fall below ``level``, linearly
        interpolated between the two lags around the crossing (``IntermediateScattering.relaxation_times``' rule); NaN for one
        that never does."""
        if self.results.get("c1") is None:
            raise RuntimeError("Analysis must be run prior to reading relaxation times")
        t = self.lag_times()
        return tuple(float(first_crossing(t, c / c[0], level)) for c in (self.results.c1, self.results.c2))
