"""Rouse normal modes and the end-to-end vector of chains on MI355X, from positions.

    X_p(c, t) = 1/N sum_{n = 1 ... N} r_n(c, t) cos(p pi (n - 1/2) / N),     p = 1 ... N - 1
    acf_p(tau) = 1/n_chains 1/(T - tau) sum_{t < T - tau} sum_c X_p(c, t) . X_p(c, t + tau)

for chains of N beads each: segmental and chain relaxation, the first diagnostic of a polymer or polyelectrolyte melt.  The
amplitudes <X_p^2> = acf_p(0) and the relaxation times tau_p are what the Rouse model predicts (both ~ 1 / sin^2(p pi / 2 N));
the end-to-end vector R = r_N - r_1 relaxes with tau_1, and <R_g^2> = 2 sum_{p >= 1} <X_p^2> (Parseval for this cosine basis).

One pass over the position slab per tile of modes (``k_chain_modes`` behind ``ta_chain_modes`` of ``include/ta_hip.h``,
hand-written HIP; a float32 slab is read as float32, never widened first) walks every chain bead by bead, makes it whole on the
way with the frame's own box, and keeps several modes in registers: a mode's coefficients sum to zero, so the functional of the
positions relative to the first bead IS the mode -- no unwrapping, and the centre of mass drops out.  The library's VACF lag
sums of the modes' columns are the autocorrelations.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from ._base import CollectiveAnalysis, first_crossing
from .compound import COMPOUND_ATTRS, compound_plan
from .orientation import group_indices  # noqa: F401  (universe indices -> positions within the group, for ``chains``)

#: modes of the default ``modes=None``: 1 ... min(N - 1, 8)
DEFAULT_MODES = 8


def rouse_coefficients(chain_len, modes):
    """(len(modes), chain_len) float64: row p holds cos(p pi (n - 1/2) / N) / N for the beads n = 1 ... N"""
    n = np.arange(1, chain_len + 1, dtype=np.float64)
    p = np.asarray(modes, dtype=np.float64)[:, None]
    return np.cos(p * np.pi * (n[None, :] - 0.5) / chain_len) / chain_len


class RouseModes(CollectiveAnalysis):
    r"""Autocorrelations of the Rouse normal modes and of the end-to-end vector of chains of equal length.

    .. math:: \mathbf{X}_p = \frac{1}{N} \sum_{n=1}^{N} \mathbf{r}_n \cos\frac{p \pi (n - 1/2)}{N}, \qquad
              C_p(\tau) = \frac{1}{n_c} \frac{1}{T - \tau} \sum_{t < T - \tau} \sum_c
              \mathbf{X}_p(c, t) \cdot \mathbf{X}_p(c, t + \tau), \qquad \langle R_g^2 \rangle = 2 \sum_{p \ge 1} \langle X_p^2 \rangle

    Parameters
    ----------
    atomgroup : AtomGroup — the trajectory must hold positions.
    chains : integer (n_chains, N) array, N >= 2 — positions WITHIN the group, every row a chain in backbone order
        (``group_indices`` maps universe indices).  The atoms of a row must differ.
    compound : one of ``'residues'``, ``'segments'``, ``'molecules'``, ``'fragments'`` — instead of ``chains``: the group's
        atoms with one label, in group order, are one chain.  Exactly one of the two is given; chains of unequal length
        raise ``ValueError``.
    modes : int P (the modes 1 ... P), a sequence of distinct integers in 1 ... N - 1, or None: 1 ... min(N - 1, 8).  p = 0 is
        the centre of mass: that is ``compound=`` of the other classes, and not offered here.
    minimum_image : bool, default True — reduce every bond by one image step per axis with the frame's own box (orthorhombic
        and triclinic; constant or per frame): the minimum image while every bond is shorter than half the smallest box width,
        so chains that the trajectory wraps across a face, bead by bead, need no unwrapping.  Every frame then needs a box.
        ``False``: the positions are used as they are.
    end_to_end : bool, default True — also the autocorrelation of R = r_N - r_1.
    fft : bool — ``True``: ``VelocityAutocorr``'s FFT evaluation for the correlations; ``False``: the direct forms.
    device, stage_dtype : keyword-only — as for the other classes.  float32 staging stays float32 on the device: the chain
        pass reads it as it is.  ``devices=[...]`` and ``distributed=True`` raise ``ValueError`` (the atoms would be split by
        index, and a chain's atoms would have to share a shard); ``by_particle=True`` raises ``TypeError``.

    Attributes
    ----------
    results.modes (P,); results.acf (P, n_frames) per chain; results.amplitude (P,) = acf[:, 0] = <X_p^2>;
    results.normalized = acf / amplitude[:, None] (NaN rows where the amplitude is 0);
    results.end_to_end_acf (n_frames,) and results.r2 = its lag 0 = <R^2> (``end_to_end``, else None);
    results.rg2 = 2 sum_p amplitude_p = <R_g^2> when the modes are exactly 1 ... N - 1, else None.
    No cross-correlation between modes and no per-chain result is formed.
    """

    _record_volumes = False
    _no_data_message = "Rouse mode computation requires positions in the trajectory"
    _updating_message = "UpdatingAtomGroups are not valid for Rouse mode computation"
    _by_particle_message = ("RouseModes has no per-particle result: the functions are sums over all chains "
                            "(by_particle=True is not supported)")

    def __init__(self, atomgroup, chains=None, *, compound=None, modes=None, minimum_image=True, end_to_end=True, fft=True,
                 **kwargs):
        for key, what in (("devices", "devices=[...]"), ("distributed", "distributed=True")):
            if kwargs.get(key):
                raise ValueError(f"RouseModes: {what} is not available -- the atoms are split over the GPUs by index, and all "
                                 "atoms of a chain would have to share a shard")
        kwargs.pop("devices", None), kwargs.pop("distributed", None)
        super().__init__(atomgroup, None, "xyz", None, fft, False, kwargs)
        if (chains is None) == (compound is None):
            raise ValueError("RouseModes: exactly one of chains= (an integer (n_chains, N) array) and compound= is expected")
        if compound is not None:
            chains = self._chains_of_compound(compound)
        c = np.asarray(chains)
        if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] < 2 or not np.issubdtype(c.dtype, np.integer):
            raise ValueError(f"chains: shape {c.shape} and dtype {c.dtype}, expected an integer (n_chains, N) array with N >= 2 "
                             "of positions within the group (chains of unequal length are not supported)")
        if c.min() < 0 or c.max() >= self.n_particles:
            raise ValueError(f"chains: entries must be positions within the group, 0 ... {self.n_particles - 1}")
        s = np.sort(c, axis=1)
        if np.any(s[:, 1:] == s[:, :-1]):
            raise ValueError(f"chains: row {int(np.flatnonzero(np.any(s[:, 1:] == s[:, :-1], axis=1))[0])} names an atom twice")
        self.chains = np.ascontiguousarray(c, dtype=np.int32)
        self.n_chains, self.chain_len = int(c.shape[0]), int(c.shape[1])
        self.modes = self._parse_modes(modes, self.chain_len)
        self.minimum_image = bool(minimum_image)
        self.end_to_end = bool(end_to_end)

    def _chains_of_compound(self, compound):
        if not isinstance(compound, str) or compound not in COMPOUND_ATTRS:
            raise ValueError(f"compound: {compound!r}, expected one of {sorted(COMPOUND_ATTRS)}")
        labels = self._group_attr(COMPOUND_ATTRS[compound], f"compound={compound!r}")
        if labels.ndim != 1 or labels.size != self.n_particles:
            raise ValueError(f"compound={compound!r}: one label per atom is expected ({self.n_particles} atoms)")
        ids, offsets, members, _ = compound_plan(labels, np.ones(labels.size))
        lengths = np.diff(offsets)
        if np.any(lengths != lengths[0]):
            raise ValueError(f"compound={compound!r}: the chains have unequal lengths ({int(lengths.min())} ... "
                             f"{int(lengths.max())} atoms); RouseModes takes chains of one length (select them)")
        return members.reshape(ids.size, int(lengths[0])).astype(np.int64)

    @staticmethod
    def _parse_modes(modes, N):
        if modes is None:
            return np.arange(1, min(N - 1, DEFAULT_MODES) + 1, dtype=np.int64)
        if isinstance(modes, (bool, np.bool_)):
            raise ValueError(f"modes: {modes!r}, expected an integer, a sequence of integers or None")
        if isinstance(modes, (int, np.integer)):
            if not 1 <= int(modes) <= N - 1:
                raise ValueError(f"modes: {int(modes)}, expected 1 ... N - 1 = {N - 1} (p = 0 is the centre of mass)")
            return np.arange(1, int(modes) + 1, dtype=np.int64)
        m = np.asarray(modes)
        if m.ndim != 1 or m.size < 1 or not np.issubdtype(m.dtype, np.integer):
            raise ValueError(f"modes: shape {m.shape} and dtype {m.dtype}, expected an integer, a sequence of integers or None")
        if m.min() < 1 or m.max() > N - 1 or np.unique(m).size != m.size:
            raise ValueError(f"modes: {[int(v) for v in m[:8]]}{' ...' if m.size > 8 else ''}, expected distinct integers in "
                             f"1 ... N - 1 = {N - 1} (p = 0 is the centre of mass)")
        return m.astype(np.int64)

    def _set_options(self, dtype):
        # float32 staging stays float32 on the device: k_chain_modes reads it as it is
        self._ctx.set_option("stage_device_f32", int(dtype == np.float32))

    @staticmethod
    def _has_data(ts):
        return ts.has_positions

    def _prepare(self):
        super()._prepare()
        self._image_boxes = np.zeros((self.n_frames, 6)) if self.minimum_image else None
        for key in ("acf", "amplitude", "normalized", "end_to_end_acf", "r2", "rg2"):
            setattr(self.results, key, None)
        self.results.modes = self.modes

    def _single_frame(self):
        if self._image_boxes is not None:
            try:
                self._image_boxes[self._frame_index] = self._unwrap_box(self._ts)
            except ValueError as err:  # (the checks of unwrap=True, under this class's keyword)
                raise ValueError(str(err).replace("unwrap=True", "minimum_image=True")) from None
        super()._single_frame()

    def coefficients(self):
        """The (n_functionals, N) matrix handed to the library: the modes' rows, then (``end_to_end``) the unit row e_N"""
        rows = [rouse_coefficients(self.chain_len, self.modes)]
        if self.end_to_end:
            e = np.zeros((1, self.chain_len))
            e[0, -1] = 1.0
            rows.append(e)
        return np.concatenate(rows, axis=0)

    def _moments(self, fft, lo, hi, correlate):
        acf = self._ctx.chain_modes(fft, self.chains, self.coefficients(), dimensions=self._image_boxes)
        return (acf,), None

    def _store(self, sums, coll):
        acf = sums[0] / float(self.n_chains)
        P = self.modes.size
        r = self.results
        r.modes = self.modes
        r.acf = acf[:P]
        r.amplitude = r.acf[:, 0].copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            r.normalized = np.where(r.amplitude[:, None] != 0, r.acf / r.amplitude[:, None], np.nan)
        r.end_to_end_acf = acf[P] if self.end_to_end else None
        r.r2 = float(acf[P, 0]) if self.end_to_end else None
        full = P == self.chain_len - 1 and np.array_equal(np.sort(self.modes), np.arange(1, self.chain_len))
        r.rg2 = float(2.0 * np.sum(r.amplitude)) if full else None

    def relaxation_times(self, level=1.0 / np.e):
        """(tau_p (P,), tau_ee): the lag times (ps) at which ``acf_p / acf_p[0]`` and the end-to-end vector's normalised
        autocorrelation first fall below ``level``, linearly interpolated between the two lags around the crossing
        (``IntermediateScattering.relaxation_times``' rule); NaN for one that never does (tau_ee also without ``end_to_end``)."""
        if self.results.get("acf") is None:
            raise RuntimeError("Analysis must be run prior to reading relaxation times")
        t = self.lag_times()
        tau = np.array([float(first_crossing(t, c, level)) if np.all(np.isfinite(c)) else np.nan for c in self.results.normalized])
        ee = self.results.end_to_end_acf
        tau_ee = float(first_crossing(t, ee / ee[0], level)) if ee is not None and ee[0] != 0 else float("nan")
        return tau, tau_ee
