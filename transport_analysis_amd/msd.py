"""Einstein mean squared displacement on MI355X — drop-in for
``MDAnalysis.analysis.msd.EinsteinMSD``.

Same constructor, ``run()`` and results as MDAnalysis' class; the per-frame position fill goes
into a pinned staging slab, and both of its evaluations (``fft=True``: the FFT form of
``tidynamics.msd``; ``fft=False``: the windowed double loop) run in hand-written HIP kernels behind
``ta_msd`` of ``include/ta_hip.h``.  Positions only: this is the path for trajectories that store
no velocities (XTC, DCD).  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from ._base import (stage_columns, AnalysisBase, NoDataError, UpdatingAtomGroup, native_rows, open_context,
                    pop_device_options, stage_frame_native)

_COMMIT_BYTES = 32 << 20

_MSD_KEYS = {
    "x": [0],
    "y": [1],
    "z": [2],
    "xy": [0, 1],
    "xz": [0, 2],
    "yz": [1, 2],
    "xyz": [0, 1, 2],
}


class EinsteinMSD(AnalysisBase):
    r"""Mean squared displacement by the Einstein relation.

    .. math:: MSD(k) = \frac{1}{N} \sum_{n} \frac{1}{T - k} \sum_{t < T - k} \sum_{d}
              (x_{t+k, n, d} - x_{t, n, d})^2

    summed over the dimensions of ``msd_type`` (no division by their number), lag 0 exactly 0.

    Parameters
    ----------
    u : Universe or AtomGroup
        Positions should be unwrapped (MDAnalysis' ``NoJump`` / ``unwrap``), as for MDAnalysis.
    select : str
        Selection applied to ``u`` (``u.select_atoms(select)``).
    msd_type : {'xyz', 'xy', 'yz', 'xz', 'x', 'y', 'z'}
        Dimensions summed over (case-insensitive).
    fft : bool
        ``True``: FFT form, O(n_frames log n_frames) (``S1 - 2 S2`` on positions shifted by their
        first frame; up to 64 frames the exact direct kernel); ``False``: the direct form.
    by_particle : bool, keyword-only, default True
        ``False`` skips ``results.msds_by_particle`` (then ``None``) and computes the lag sums only.
    device, devices, distributed, stage_dtype : keyword-only
        As for ``VelocityAutocorr``: a GPU index or ``"cpu"`` (the opt-in C++/OpenMP backend),
        several GPUs behind one object, or one process per GPU under ``torch.distributed``
        (``results.msds_by_particle`` then holds this rank's atoms, ``results.particle_range``).

    Attributes
    ----------
    results.timeseries : (n_frames,) float64 — MSD averaged over particles (Å^2).
    results.msds_by_particle : (n_frames, n_particles) float64 or None
    ag, n_particles, fft, msd_type, dim_fac, select
    """

    def __init__(self, u, select="all", msd_type="xyz", fft=True, **kwargs):
        if isinstance(u, UpdatingAtomGroup):
            raise TypeError("UpdatingAtomGroups are not valid for MSD computation")
        self._want_by_particle = bool(kwargs.pop("by_particle", True))
        self._stage_dtype = kwargs.pop("stage_dtype", None)
        self._distributed, self._devices, self._device = pop_device_options(kwargs)
        super().__init__(u.universe.trajectory, **kwargs)

        self.u = u
        self.msd_type = msd_type
        self._parse_msd_type()
        self.select = select
        self.fft = fft
        self.ag = u.select_atoms(self.select)
        self.n_particles = len(self.ag)
        self._ctx = None
        self.results.msds_by_particle = None
        self.results.timeseries = None

    def _parse_msd_type(self):
        """Columns and dimensionality factor of msd_type, with MDAnalysis' error."""
        self.msd_type = self.msd_type.lower()
        try:
            self._dim = list(_MSD_KEYS[self.msd_type])
        except KeyError:
            raise ValueError(
                "invalid msd_type: {} specified, please specify one of xyz, "
                "xy, xz, yz, x, y, z".format(self.msd_type)
            )
        self.dim_fac = len(self._dim)

    # frames are staged into one device slab and every lag couples all frames: atoms, not frames, are the
    # parallel axis of this path (distributed=True)
    _analysis_algorithm_is_parallelizable = False

    @classmethod
    def get_supported_backends(cls):
        return ("serial",)

    def _pick_stage_dtype(self):
        """float32 when the trajectory hands out float32 positions (MDAnalysis does): lossless, half
        the PCIe bytes; the device slab and all arithmetic are float64."""
        if self._stage_dtype is not None:
            return np.dtype(self._stage_dtype)
        try:
            dt = np.asarray(self.ag.positions).dtype
        except Exception:  # no positions: _single_frame raises NoDataError
            return np.dtype(np.float64)
        return np.dtype(np.float32) if dt == np.float32 else np.dtype(np.float64)

    # ------------------------------------------------------------ hooks
    def _prepare(self):
        """Pinned host slab + device slab instead of MDAnalysis' ``np.zeros`` position array."""
        if self._ctx is None:
            self._ctx = open_context(self._devices, self._device)
        self._ctx.set_option("stage_device_f32", 0)
        self._lo, self._hi = 0, self.n_particles
        self._source = self.ag
        if self._distributed:
            from .dist import shard_of_this_rank

            _, _, self._lo, self._hi = shard_of_this_rank(self.n_particles)
            self.results.particle_range = (self._lo, self._hi)
            self._source = self.ag[self._lo:self._hi]
        self._n_local = self._hi - self._lo
        dtype = self._pick_stage_dtype()
        if self._devices is not None:
            (views,) = self._ctx.stage_alloc(self.n_frames, self.n_particles, self.dim_fac, n_slabs=1, dtype=dtype)
            self._targets = [(v, lo, hi) for v, (lo, hi) in zip(views, self._ctx.shards) if hi > lo]
            self.results.device_ranges = list(self._ctx.shards)
        else:
            (view,) = self._ctx.stage_alloc(self.n_frames, max(self._n_local, 1), self.dim_fac, n_slabs=1, dtype=dtype)
            self._targets = [(view, 0, self._n_local)] if self._distributed else [(view, self._lo, self._hi)]
        self._rows = native_rows(self._source) if self._n_local else None
        frame_bytes = max(1, self._n_local * self.dim_fac * dtype.itemsize)
        self._commit_every = max(1, _COMMIT_BYTES // frame_bytes)
        self._committed = 0
        self.results.msds_by_particle = None
        self.results.timeseries = None
        self._bp_home = None
        if self._want_by_particle and self._n_local and not self._device_reduce():
            self._bp_home = self._ctx.result_home((self.n_frames, self._n_local))

    def _single_frame(self):
        """Stage the selected position columns of one frame."""
        if not self._ts.has_positions:
            raise NoDataError("MSD computation requires positions in the trajectory")
        i = self._frame_index
        if self._n_local and not stage_frame_native(self._ctx, 0, i, self._ts, "positions", self._dim, self._rows):
            pos = np.asarray(self._source.positions)
            for view, lo, hi in self._targets:
                stage_columns(view[i], pos, lo, hi, self._dim)
        if i + 1 - self._committed >= self._commit_every:
            self._ctx.stage_commit(self._committed, i + 1)
            self._committed = i + 1

    def _conclude(self):
        if self._committed < self.n_frames:
            self._ctx.stage_commit(self._committed, self.n_frames)
            self._committed = self.n_frames
        if self._device_reduce():  # RCCL: the lag sums stay on the GPU through the reduce
            from .dist import staged_timeseries_on_device

            ts, bp = staged_timeseries_on_device(self._ctx, "msd", self.n_frames, self._n_local, self.n_particles,
                                                 self._device, by_particle=self._want_by_particle, fft=bool(self.fft))
        else:
            home = self._bp_home.get() if self._bp_home is not None else None
            self._bp_home = None
            ts, bp = self._ctx.msd(bool(self.fft), by_particle=self._want_by_particle, out=home)
            if self._distributed:
                from .dist import allreduce_mean_over_atoms

                if self._n_local == 0:  # more ranks than atoms: this rank contributes nothing
                    ts, bp = np.zeros(self.n_frames), (None if bp is None else bp[:, :0])
                ts = allreduce_mean_over_atoms(ts, self._n_local, self.n_particles, self._device)
        self.results.msds_by_particle = bp
        self.results.timeseries = ts

    def _device_reduce(self):
        if not self._distributed:
            return False
        from .dist import uses_device_reduce

        return uses_device_reduce()
