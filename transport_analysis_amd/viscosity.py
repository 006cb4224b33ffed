"""Einstein-Helfand viscosity function on MI355X — drop-in for
``transport_analysis.viscosity.ViscosityHelfand``
(/root/reference/transport_analysis/viscosity.py:26-272).  The windowed
mean-squared-difference accumulator of ``_conclude`` (:201-233) runs in a
hand-written HIP kernel; the fit (:235-245) stays on the host.  No CPU fallback.
"""
from __future__ import annotations

import functools

import numpy as np

from ._base import BOLTZMANN, StagedAnalysis, UpdatingAtomGroup, parse_dim_type


class ViscosityHelfand(StagedAnalysis):
    r"""Viscosity function via the Einstein-Helfand method.

    Parameters
    ----------
    atomgroup : AtomGroup
    temp_avg : float — average temperature (K), default 300.
    dim_type : {'xyz', 'xy', 'yz', 'xz', 'x', 'y', 'z'}
    linear_fit_window : (int, int) or None — lag-index window for the slope fit.
    by_particle : bool, keyword-only, default True — materialise
        ``results.visc_by_particle``; ``False`` computes the timeseries only.  Both run on the
        matrix cores (FP64; ``float32=True``: FP32), every lag to the path's accuracy.
    device : int or "cpu", keyword-only — GPU index (default ``$TA_AMD_DEVICE`` or 0); ``"cpu"`` asks
        for the library's opt-in CPU backend (C++/OpenMP behind the same C symbols; nothing selects it
        on the caller's behalf).
    distributed : bool, keyword-only, default False — one process per GPU under
        ``torch.distributed``: each rank handles its contiguous block of atoms, one all-reduce of
        the lag sums gives ``results.timeseries`` on every rank; ``results.visc_by_particle``
        holds this rank's atoms only (``results.particle_range``).
    float32 : bool, keyword-only, default False — form the mass-weighted
        velocity-position products in float64, then evaluate the squared differences and
        their block sums in float32 (accumulated into float64): 2e-6 of the series' scale
        instead of 1e-10 relative, 1.9x the throughput.  The products are rounded to float32
        ONCE before differences are formed, so the shortest lags of a smooth, trending series see
        that rounding (6e-8 of |P|) against a small difference: on the reference's step trajectory
        1e-5 relative at lag 1, 2e-6 at lags 2-4, 3e-7 from lag 5 on; a fit window that starts at
        lag 5 or later is unaffected.  (The CPU backend computes this option in float64.)

    fft : bool, keyword-only, default False — an extension (the reference has only the
        O(n_frames^2) loop): evaluate the mean squared differences in
        O(n_frames log n_frames) as ``S1(k) - 2 S2(k)`` (``S2`` = FFT autocorrelation of the
        products ``m v x``, ``S1`` from prefix sums), with or without the per-particle array, for
        n_frames <= 163840 (longer trajectories fall back to the direct correlator).  Accurate to ~1e-15 of the series' scale;
        lags whose mean squared difference is far below the squared products themselves lose
        relative accuracy by that ratio.

    Attributes
    ----------
    results.timeseries : (n_frames,) — viscosity function averaged over particles
        (lag 0 is exactly 0).
    results.visc_by_particle : (n_frames, n_particles) or None
    results.viscosity : slope of the linear fit (only with linear_fit_window).
    """

    _stage_arrays = ("velocities", "positions")
    _by_particle_key = "visc_by_particle"
    _record_volumes = True
    _no_data_message = ("Helfand viscosity computation requires "
                        "velocities, positions, and box volume in the trajectory")

    def __init__(self, atomgroup, temp_avg=300.0, dim_type="xyz", linear_fit_window=None,
                 **kwargs):
        super().__init__(atomgroup, **kwargs)

        if isinstance(atomgroup, UpdatingAtomGroup):
            raise TypeError("UpdatingAtomGroups are not valid for viscosity computation")

        self.temp_avg = temp_avg
        self.dim_type = dim_type.lower()
        self.linear_fit_window = linear_fit_window
        self._dim, self.dim_fac = parse_dim_type(self.dim_type)

        self.atomgroup = self._group = atomgroup
        self.n_particles = len(self.atomgroup)

    def _pop_options(self, kwargs):
        self._float32 = bool(kwargs.pop("float32", False))
        self._fft = bool(kwargs.pop("fft", False))
        if self._fft and self._float32:
            raise ValueError("fft=True and float32=True are exclusive")

    _parse_dim_type = staticmethod(parse_dim_type)

    def _set_options(self, dtype):
        self._ctx.set_option("direct_f32", int(self._float32))
        self._ctx.set_option("helfand_fft", int(self._fft))
        # float32 path: the device slabs keep float32 staging as float32 (half the footprint; the
        # kernels round the staged value to float32 anyway, so the results do not change)
        self._ctx.set_option("stage_device_f32", int(self._float32))

    def _prepare(self):
        """Two pinned slabs (velocities, positions) + volumes + masses (:111-142)."""
        super()._prepare()
        self._masses = np.asarray(self.atomgroup.masses, dtype=np.float64)[self._lo:self._hi]
        if self._n_local == 0:
            self._masses = np.ones(1)
        self.boltzmann = BOLTZMANN

    @staticmethod
    def _has_data(ts):
        return ts.has_velocities and ts.has_positions and ts.volume != 0

    def _evaluate(self):
        # everything is divided by 2 kB <V> T (:229-231)
        scale = 1.0 / (2 * self.boltzmann * self._vol_avg * self.temp_avg)

        def launch(d_lagsum, d_bp, ld_bp, stream):
            import torch

            m = torch.as_tensor(np.ascontiguousarray(self._masses, dtype=np.float64),
                                device=torch.device("cuda", self._device))
            self._ctx.helfand_msd_staged(m.data_ptr(), float(scale), d_lagsum, d_bp, ld_bp, stream)
            return m  # kept alive until the results are back on the host

        self._run_kernels(functools.partial(self._ctx.helfand_msd, self._masses, scale), launch)

        if self.linear_fit_window is not None:
            # the reference fits against lagtimes = arange(1, n_frames): its x axis
            # is one ahead of the timeseries index; the slope is unaffected (:235-245)
            lagtimes = np.arange(1, self.n_frames)
            lo, hi = self.linear_fit_window[0], self.linear_fit_window[1]
            fit = np.polyfit(lagtimes[lo:hi], self.results.timeseries[lo:hi], 1)
            self.results.viscosity = fit[0]

    def plot_viscosity_function(self):
        """Plot the viscosity function against lag index, marking the fit window (:247-272)."""
        import matplotlib.pyplot as plt

        plt.plot(np.arange(0, self.n_frames), self.results.timeseries, label="Viscosity Function")
        if self.linear_fit_window is not None:
            lo, hi = self.linear_fit_window[0], self.linear_fit_window[1]
            plt.axvline(lo, color="red", linestyle="--", label="Fit Start")
            plt.axvline(hi, color="blue", linestyle="--", label="Fit End")
        plt.xlabel("Lag-time")
        plt.ylabel("Viscosity Function")
        plt.title("Viscosity Function vs Lag-time")
        plt.legend()
        plt.show()
