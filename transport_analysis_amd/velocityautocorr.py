"""Velocity autocorrelation function on MI355X — drop-in for
``transport_analysis.velocityautocorr.VelocityAutocorr``.

Same constructor, ``run()``, results and helper methods as the reference
(/root/reference/transport_analysis/velocityautocorr.py:72-422); the arithmetic
of ``_conclude_fft`` (:208-215) and ``_conclude_simple`` (:217-238) runs in
hand-written HIP kernels behind the C-ABI of ``include/ta_hip.h``.  There is no
CPU fallback.
"""
from __future__ import annotations

import numpy as np

from ._base import StagedAnalysis, UpdatingAtomGroup, parse_dim_type


class VelocityAutocorr(StagedAnalysis):
    r"""Velocity autocorrelation function (VACF) of an AtomGroup.

    Parameters
    ----------
    atomgroup : AtomGroup
        Particles to analyse.  An ``UpdatingAtomGroup`` raises ``TypeError``.
    dim_type : {'xyz', 'xy', 'yz', 'xz', 'x', 'y', 'z'}
        Dimensions included in the VACF (case-insensitive, order-sensitive).
    fft : bool
        ``True``: FFT algorithm (reference: ``tidynamics.acf`` per atom);
        ``False``: direct "windowed" algorithm.  Both give the same quantity.
    by_particle : bool, keyword-only, default True
        ``True`` materialises ``results.vacf_by_particle`` (n_frames, n_atoms)
        as the reference does (``fft=False``: on the FP64 matrix cores, a particle's
        column in a per-wave LDS ring).  ``False`` computes only
        ``results.timeseries`` (``fft=True``: power spectra are summed
        over atoms on the GPU before the single inverse transform, 2.4x faster;
        ``fft=False``: the lag sums are the diagonal sums of the frames' Gram matrix,
        on the FP64 matrix cores, no faster than with the array) and
        ``results.vacf_by_particle`` is ``None``.
    device : int or "cpu", keyword-only
        GPU index (default: ``$TA_AMD_DEVICE`` or 0; with ``distributed=True``:
        ``$TA_AMD_DEVICE``, else ``$LOCAL_RANK``, else torch's current device).  ``"cpu"`` (or
        ``$TA_AMD_DEVICE=cpu``) asks for the library's opt-in CPU backend -- C++/OpenMP behind the
        same C symbols (``csrc/cpu_backend.cpp``); it is never selected on the caller's behalf: without
        a GPU every other value fails loudly.
    stage_dtype : numpy dtype, keyword-only
        Element type of the pinned staging slab.  Default: the dtype MDAnalysis hands the
        velocities out in (float32) -- lossless, half the PCIe bytes of the reference's
        float64 slab; the device slab and all arithmetic are float64 either way.
    device_float32 : bool or None, keyword-only, default None
        Keep float32-staged frames as float32 in the DEVICE slab as well (half the device memory:
        12 GB instead of 24 GB at 10000 frames x 100000 atoms; the FFT kernels read the 8-byte rows
        and widen them exactly, 3-14 % faster than from float64 slabs; same values in, results
        equal to float64 slabs within 1e-15 of the scale).  ``None``: on when the staging slab is
        float32, ``fft=True`` and the trajectory has 513 ... 10240 frames (the plans that read
        float32 rows; any other evaluation of float32 device slabs first widens them).
    devices : sequence of int, keyword-only
        Several GPUs from ONE process and ONE pass over the trajectory: the
        atoms are split into contiguous blocks, one per GPU; every frame's columns go straight
        into each GPU's pinned slab, the kernels run on all GPUs at once, the lag sums are reduced
        once inside the library (RCCL) and ``results.vacf_by_particle`` is ONE
        ``(n_frames, n_particles)`` array whose column ranges the GPUs fill.  The script is the
        reference's, unchanged.  Exclusive with ``distributed``.
    distributed : bool, keyword-only, default False
        One process per GPU under ``torch.distributed`` (e.g. ``torchrun``): every rank runs
        the same script on the same AtomGroup, stages and correlates only its contiguous block
        of atoms (and asks the trajectory for that block's velocities only) and ONE all-reduce of
        the lag sums gives ``results.timeseries`` (the mean over ALL atoms) on every rank.
        ``results.vacf_by_particle`` then holds this rank's atoms only,
        ``results.particle_range = (lo, hi)``.

    Attributes
    ----------
    results.timeseries : (n_frames,) float64 — VACF averaged over particles,
        lag index k = 0..n_frames-1, units (Å/ps)^2.
    results.vacf_by_particle : (n_frames, n_particles) float64 or None
    dim_fac, n_frames, n_particles, times, frames, start, stop, step
    """

    _stage_arrays = ("velocities",)
    _by_particle_key = "vacf_by_particle"
    _no_data_message = "VACF computation requires velocities in the trajectory"

    def __init__(self, atomgroup, dim_type="xyz", fft=True, **kwargs):
        super().__init__(atomgroup, **kwargs)

        if isinstance(atomgroup, UpdatingAtomGroup):
            raise TypeError("UpdatingAtomGroups are not valid for VACF computation")

        self.dim_type = dim_type.lower()
        self._dim, self.dim_fac = parse_dim_type(self.dim_type)
        self.fft = fft

        self.atomgroup = self._group = atomgroup
        self.n_particles = len(self.atomgroup)
        self._run_called = False

    def _pop_options(self, kwargs):
        self._device_f32 = kwargs.pop("device_float32", None)

    _parse_dim_type = staticmethod(parse_dim_type)

    # ------------------------------------------------------------ hooks
    # _prepare (:142-153; results.timeseries is not set there) and _single_frame (:178-194) are
    # StagedAnalysis': the velocity columns go into a pinned host slab and on to the device.
    @staticmethod
    def _has_data(ts):
        return ts.has_velocities

    def _set_options(self, dtype):
        dev32 = self._device_f32
        if dev32 is None:  # float32 staging stays float32 on the device where the FFT kernels read it as it is
            dev32 = dtype == np.float32 and bool(self.fft) and 512 < self.n_frames <= 10240
        self._ctx.set_option("stage_device_f32", int(bool(dev32) and dtype == np.float32))

    def _evaluate(self):
        if self.fft:
            self._conclude_fft()
        else:
            self._conclude_simple()
        self._run_called = True

    def _conclude_fft(self):
        self._run_kernels(self._ctx.vacf_fft, lambda *a: self._ctx.vacf_fft_staged(*a))

    def _conclude_simple(self):
        self._run_kernels(self._ctx.vacf_direct, lambda *a: self._ctx.vacf_direct_staged(*a))

    # --------------------------------------------- post-processing (host)
    def _window(self, start, stop, step):
        stop = self.n_frames if stop == 0 else stop
        sl = slice(start, stop, step)
        return self.times[sl], self.results.timeseries[sl]

    def plot_vacf(self, start=0, stop=0, step=1, xlabel="Time (ps)",
                  ylabel="Velocity Autocorrelation Function (Å^2 / ps^2)"):
        """Plot the VACF (:240-285).  Returns the list of Line2D from ``Axes.plot``."""
        if not self._run_called:
            raise RuntimeError("Analysis must be run prior to plotting")
        import matplotlib.pyplot as plt

        t, y = self._window(start, stop, step)
        _, ax = plt.subplots()
        ax.set_xlabel(xlabel)
        ax.set_ylabel(ylabel)
        return ax.plot(t, y)

    def self_diffusivity_gk(self, start=0, stop=0, step=1):
        """Green-Kubo self-diffusivity, trapezoid rule, divided by dim_fac (:287-322)."""
        if not self._run_called:
            raise RuntimeError("Analysis must be run prior to computing self-diffusivity")
        from scipy import integrate

        t, y = self._window(start, stop, step)
        return integrate.trapezoid(y, t) / self.dim_fac

    def self_diffusivity_gk_odd(self, start=0, stop=0, step=1):
        """Green-Kubo self-diffusivity, Simpson rule (:324-360)."""
        if not self._run_called:
            raise RuntimeError("Analysis must be run prior to computing self-diffusivity")
        from scipy import integrate

        t, y = self._window(start, stop, step)
        return integrate.simpson(y=y, x=t) / self.dim_fac

    def plot_running_integral(self, start=0, stop=0, step=1, initial=0, xlabel="Time (ps)",
                              ylabel="Running Integral of the VACF (Å^2 / ps)"):
        """Plot the cumulative trapezoid integral of the VACF / dim_fac (:362-422)."""
        if not self._run_called:
            raise RuntimeError("Analysis must be run prior to plotting")
        import matplotlib.pyplot as plt
        from scipy import integrate

        t, y = self._window(start, stop, step)
        running = integrate.cumulative_trapezoid(y, t, initial=initial) / self.dim_fac
        _, ax = plt.subplots()
        ax.set_xlabel(xlabel)
        ax.set_ylabel(ylabel)
        return ax.plot(t, running)
