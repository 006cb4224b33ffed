"""Self part of the van Hove function G_s(r, t) and the non-Gaussian parameter alpha_2(t) on MI355X, from positions.

    G_s(r, tau) = 1/N < sum_n delta(r - |x_n(t0 + tau) - x_n(t0)|) >        (the distribution of displacements after a lag)
    alpha_2(tau) = d / (d + 2) <dr^4> / <dr^2>^2 - 1                        (0 for the Gaussian that EinsteinMSD assumes)

averaged over time origins t0.  It is the real-space partner of ``IntermediateScattering``: F_s(k, t) is the Fourier
transform of G_s(r, t).  A histogram is no correlation and has no FFT form: one pass over the position slab per chunk of
lags (``k_vanhove`` behind ``ta_vanhove`` of ``include/ta_hip.h``, hand-written HIP; a float32 slab is read as float32,
never widened first) counts the squared displacements against squared bin edges in integer histograms and adds their
second and fourth moments in a fixed order.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from ._base import CollectiveAnalysis

#: TA_VANHOVE_MAX_LAGS, TA_VANHOVE_MAX_BINS of include/ta_hip.h
MAX_LAGS, MAX_BINS = 1024, 4096


def log_lags(n_frames, per_decade=8):
    """Logarithmically spaced integer frame lags: the sorted unique ``int(round(10**(i / per_decade)))`` below
    ``n_frames``, starting at 1, at most ``TA_VANHOVE_MAX_LAGS`` of them (empty for fewer than two frames)."""
    n_frames, per_decade = int(n_frames), int(per_decade)
    if per_decade < 1:
        raise ValueError("per_decade must be >= 1")
    out, i = [], 0
    while True:
        lag = int(round(10.0 ** (i / per_decade)))
        if lag >= n_frames:
            break
        if not out or lag > out[-1]:
            out.append(lag)
        i += 1
    return np.array(out[:MAX_LAGS], dtype=np.int64)


def _check_lags(lags, n_frames=None):
    lg = np.asarray(lags)
    if lg.ndim != 1 or lg.size < 1 or not np.issubdtype(lg.dtype, np.integer):
        raise ValueError(f"lags: a non-empty 1-d sequence of integer frame lags is expected, got shape {lg.shape} and dtype {lg.dtype}")
    lg = lg.astype(np.int64)
    if lg.size > MAX_LAGS:
        raise ValueError(f"lags: {lg.size} lags, at most {MAX_LAGS}")
    if lg[0] < 0 or np.any(np.diff(lg) <= 0):
        raise ValueError("lags must be >= 0 and strictly increasing")
    if n_frames is not None and lg[-1] >= n_frames:
        raise ValueError(f"lags: lag {int(lg[-1])} needs more than the {n_frames} analysed frames")
    return lg


class _VanHove(CollectiveAnalysis):
    """What ``VanHoveSelf`` and ``VanHoveDistinct`` share: the bins, the lags and the grid half of the results."""

    _no_data_message = "Van Hove function computation requires positions in the trajectory"
    _updating_message = "UpdatingAtomGroups are not valid for van Hove function computation"

    def __init__(self, atomgroup, lags, r_max, n_bins, dim_type, unwrap, kwargs):
        super().__init__(atomgroup, None, dim_type, None, False, unwrap, kwargs)
        self.r_max, self.n_bins = float(r_max), int(n_bins)
        if not np.isfinite(self.r_max) or not self.r_max > 0:
            raise ValueError(f"r_max must be finite and > 0, got {r_max}")
        if not 1 <= self.n_bins <= MAX_BINS:
            raise ValueError(f"n_bins must be 1 ... {MAX_BINS}, got {n_bins}")
        self.dr = self.r_max / self.n_bins
        self.lags = None if lags is None else _check_lags(lags)

    def _set_options(self, dtype):
        # float32 staging stays float32 on the device: the kernels read it as it is (the unwrap pass works on float64 slabs)
        self._ctx.set_option("stage_device_f32", int(dtype == np.float32 and not self._unwrap))

    @staticmethod
    def _has_data(ts):
        return ts.has_positions

    def _prepare(self):
        # (before the slabs are allocated: the number of analysed frames is known here, the trajectory is not read yet)
        self._lags = self._default_lags() if self.lags is None else _check_lags(self.lags, self.n_frames)
        super()._prepare()
        for key in self._result_keys:
            setattr(self.results, key, None)

    def _correlate(self, fft, sums):
        return None  # the sums are the result: there is no correlation step

    def _store_grid(self, counts):
        """lags, times, bin_edges, r, counts and overflow of the (L, B + 1) int64 ``counts``; returns the (B,) measures
        of the shells between the edges (4 pi / 3 (r+^3 - r-^3), pi (r+^2 - r-^2), 2 dr for d = 3, 2, 1)"""
        r = self.results
        B, dr = self.n_bins, self.dr
        r.lags = self._lags
        r.times = self._lags * (float(self.times[1] - self.times[0]) if self.n_frames > 1 else 0.0)
        r.bin_edges = np.arange(B + 1) * dr
        r.r = 0.5 * (r.bin_edges[1:] + r.bin_edges[:-1])
        r.counts, r.overflow = np.ascontiguousarray(counts[:, :B]), counts[:, B].copy()
        lo, hi = r.bin_edges[:-1], r.bin_edges[1:]
        return {3: 4.0 * np.pi / 3.0 * (hi ** 3 - lo ** 3), 2: np.pi * (hi ** 2 - lo ** 2), 1: np.full(B, 2.0 * dr)}[self.dim_fac]


class VanHoveSelf(_VanHove):
    r"""Self van Hove function and non-Gaussian parameter of a group of atoms (or of molecules' centres).

    .. math:: G_s(r, \tau) = \frac{1}{N (T - \tau)} \sum_{t < T - \tau} \sum_n
              \delta(r - |\mathbf{x}_n(t + \tau) - \mathbf{x}_n(t)|), \qquad
              \alpha_2(\tau) = \frac{d}{d + 2} \frac{\langle \Delta r^4 \rangle}{\langle \Delta r^2 \rangle^2} - 1

    Parameters
    ----------
    atomgroup : AtomGroup — the trajectory must hold positions.
    lags : integer frame lags, strictly increasing, below the number of analysed frames; ``None`` (the default):
        ``log_lags(n_frames, per_decade=8)``.
    r_max, n_bins : keyword-only — ``n_bins`` bins of width ``dr = r_max / n_bins`` on [0, r_max); displacements beyond
        are counted in ``results.overflow``.
    dim_type : {'xyz', 'xy', 'yz', 'xz', 'x', 'y', 'z'} — d, the number of analysed dimensions, follows.
    unwrap : bool, default False — undo periodic wrapping first (``EinsteinMSD``'s); wrapped positions give wrong
        displacements.
    compound, compound_weights, reference_frame : keyword-only — as for ``EinsteinMSD``: the displacements of molecules'
        centres; N is then the number of compounds.
    device, devices, distributed, stage_dtype : keyword-only — as for the other classes.  float32 staging stays float32
        on the device (unless ``unwrap=True``, which works on float64 slabs).  Counts and moments add up over atoms:
        under ``distributed=True`` and ``devices=[...]`` the blocks' sums are added.
    A box is needed only for ``unwrap``.  ``by_particle=True`` raises ``TypeError``.

    Attributes
    ----------
    With ``n_pairs[l] = N (T - lags[l])``: results.lags (L,); results.times (L,) ps; results.bin_edges (B + 1,); results.r
    (B,) the bin centres; results.counts (L, B) int64; results.overflow (L,); results.prob (L, B) = counts / (n_pairs dr),
    the density of \|dr\| (``sum(prob) dr + overflow / n_pairs = 1``); results.gs (L, B) = counts / (n_pairs V_b), V_b the
    measure of the shell between the edges (4 pi / 3 (r+^3 - r-^3), pi (r+^2 - r-^2), 2 dr for d = 3, 2, 1); results.msd
    (L,) and results.r4 (L,) the second and fourth moments; results.alpha2 (L,), NaN where msd is 0.
    """

    _accepts_compound = True
    _record_volumes = False
    _by_particle_message = ("VanHoveSelf has no per-particle result: the histograms are sums over all atoms "
                            "(by_particle=True is not supported)")
    _result_keys = ("lags", "times", "bin_edges", "r", "counts", "overflow", "prob", "gs", "msd", "r4", "alpha2")

    def __init__(self, atomgroup, lags=None, *, r_max, n_bins=200, dim_type="xyz", unwrap=False, **kwargs):
        super().__init__(atomgroup, lags, r_max, n_bins, dim_type, unwrap, kwargs)

    def _default_lags(self):
        lags = log_lags(self.n_frames)
        if lags.size == 0:
            raise ValueError(f"lags=None needs at least two analysed frames, got {self.n_frames}")
        return lags

    def _moments(self, fft, lo, hi, correlate):
        return self._ctx.vanhove(self._lags, self.n_bins, self.dr), None

    def _no_moments(self):
        L = self._lags.size
        return np.zeros((L, self.n_bins + 1)), np.zeros((L, 2))

    def _store(self, sums, _):
        # (under distributed=True the counts have travelled as float64 through the all-reduce: integers below 2^53 are
        # exact there, and a count is at most N T, far below that)
        shell = self._store_grid(np.rint(sums[0]).astype(np.int64))
        moments = np.asarray(sums[1], dtype=np.float64)
        r, d = self.results, self.dim_fac
        n_pairs = (float(self.n_particles) * (self.n_frames - self._lags)).astype(np.float64)
        r.prob = r.counts / (n_pairs[:, None] * self.dr)
        r.gs = r.counts / (n_pairs[:, None] * shell[None, :])
        r.msd, r.r4 = moments[:, 0] / n_pairs, moments[:, 1] / n_pairs
        with np.errstate(divide="ignore", invalid="ignore"):
            r.alpha2 = np.where(r.msd == 0, np.nan, d / (d + 2.0) * r.r4 / r.msd ** 2 - 1.0)

    def gaussian_reference(self):
        """(L, B) the Gaussian G_s with the same msd at the bin centres, (d / (2 pi msd))^(d / 2) exp(-d r^2 / (2 msd)):
        what ``results.gs`` is when ``alpha2`` is 0 (NaN rows where msd is 0)."""
        if self.results.get("msd") is None:
            raise RuntimeError("Analysis must be run prior to reading the Gaussian reference")
        d = self.dim_fac
        with np.errstate(divide="ignore", invalid="ignore"):
            msd = np.where(self.results.msd == 0, np.nan, self.results.msd)[:, None]
            return (d / (2.0 * np.pi * msd)) ** (d / 2.0) * np.exp(-d * self.results.r[None, :] ** 2 / (2.0 * msd))
