"""Einstein mean squared displacement on MI355X — drop-in for
``MDAnalysis.analysis.msd.EinsteinMSD``.

Same constructor, ``run()`` and results as MDAnalysis' class; the per-frame position fill goes
into a pinned staging slab, and both of its evaluations (``fft=True``: the FFT form of
``tidynamics.msd``; ``fft=False``: the windowed double loop) run in hand-written HIP kernels behind
``ta_msd`` of ``include/ta_hip.h``.  Positions only: this is the path for trajectories that store
no velocities (XTC, DCD).  There is no CPU fallback.
"""
from __future__ import annotations

import functools

from ._base import StagedAnalysis, UpdatingAtomGroup, parse_dim_type


class EinsteinMSD(StagedAnalysis):
    r"""Mean squared displacement by the Einstein relation.

    .. math:: MSD(k) = \frac{1}{N} \sum_{n} \frac{1}{T - k} \sum_{t < T - k} \sum_{d}
              (x_{t+k, n, d} - x_{t, n, d})^2

    summed over the dimensions of ``msd_type`` (no division by their number), lag 0 exactly 0.

    Parameters
    ----------
    u : Universe or AtomGroup
        Positions must be unwrapped for a meaningful MSD: pass ``unwrap=True`` for a trajectory written
        wrapped into the box, or unwrap beforehand (MDAnalysis' ``NoJump``).
    select : str
        Selection applied to ``u`` (``u.select_atoms(select)``).
    msd_type : {'xyz', 'xy', 'yz', 'xz', 'x', 'y', 'z'}
        Dimensions summed over (case-insensitive).
    fft : bool
        ``True``: FFT form, O(n_frames log n_frames) (``S1 - 2 S2`` on positions shifted by their
        first frame; up to 64 frames the exact direct kernel); ``False``: the direct form.
    by_particle : bool, keyword-only, default True
        ``False`` skips ``results.msds_by_particle`` (then ``None``) and computes the lag sums only.
    unwrap : bool, keyword-only, default False
        ``True``: undo the periodic wrapping of the staged positions on the device before the MSD, as
        MDAnalysis' ``NoJump`` does (``ta_unwrap``: image counts from the jumps of the fractional
        coordinates between consecutive analysed frames, an exact integer prefix sum along time; frame 0
        is kept as it is; a box that changes from frame to frame is followed).  Every analysed frame needs
        a box (``ts.dimensions``) with lengths > 0, else ``ValueError``; a non-orthogonal box needs
        ``msd_type='xyz'``, else ``ValueError``.  Analysed frames that are not consecutive (``step > 1``,
        ``frames=``) give a ``UserWarning`` and are unwrapped over the analysed frames.  A particle that moves
        more than half a box between two analysed frames cannot be unwrapped (not detected).  ``False``
        (default): the positions are used as they are.
    compound : keyword-only, default None
        ``None``: the MSD of atoms.  ``"residues"``, ``"segments"``, ``"molecules"``, ``"fragments"`` (the group's
        ``resindices``, ``segindices``, ``molnums``, ``fragindices``) or one integer label per atom: the MSD of the
        weighted centre of every compound.  The frames are staged (and unwrapped) as atoms; one pass on the device
        (``k_compound`` behind ``ta_compound``) then replaces the slab by the compounds'.  ``n_particles``,
        ``results.msds_by_particle`` and the mean are those of the compounds, ``results.compound_ids`` their labels
        (``np.unique`` order).
    compound_weights : keyword-only, default ``"mass"``
        ``"mass"`` (the group's ``masses``: centres of mass), ``"geometry"`` (equal weights) or one value per atom;
        normalised within every compound.
    reference_frame : keyword-only, default None
        ``"barycentric"``: positions relative to the centre of mass of all atoms of the group, frame by frame (allowed
        with ``compound=None``: every atom is then its own compound).
        None of the three is available with ``devices=[...]`` or ``distributed=True`` (``ValueError``): the atoms of a
        molecule would have to share a shard.
    device, devices, distributed, stage_dtype : keyword-only
        As for ``VelocityAutocorr``: a GPU index or ``"cpu"`` (the opt-in C++/OpenMP backend),
        several GPUs behind one object, or one process per GPU under ``torch.distributed``
        (``results.msds_by_particle`` then holds this rank's atoms, ``results.particle_range``).

    Attributes
    ----------
    results.timeseries : (n_frames,) float64 — MSD averaged over particles (Å^2).
    results.msds_by_particle : (n_frames, n_particles) float64 or None
    ag, n_particles, fft, msd_type, dim_fac, select, unwrap
    """

    _stage_arrays = ("positions",)
    _by_particle_key = "msds_by_particle"
    _no_data_message = "MSD computation requires positions in the trajectory"
    _accepts_compound = True

    def __init__(self, u, select="all", msd_type="xyz", fft=True, *, unwrap=False, **kwargs):
        if isinstance(u, UpdatingAtomGroup):
            raise TypeError("UpdatingAtomGroups are not valid for MSD computation")
        super().__init__(u, **kwargs)
        self._unwrap = bool(unwrap)

        self.u = u
        self.msd_type = msd_type
        self._parse_msd_type()
        self.select = select
        self.fft = fft
        self.unwrap = self._unwrap
        self.ag = self._group = u.select_atoms(self.select)
        self.n_particles = len(self.ag)
        self._init_compound()
        self.results.msds_by_particle = None
        self.results.timeseries = None

    def _parse_msd_type(self):
        """Columns and dimensionality factor of msd_type, with MDAnalysis' error."""
        self.msd_type = self.msd_type.lower()
        self._dim, self.dim_fac = parse_dim_type(self.msd_type, "msd_type")

    # ------------------------------------------------------------ hooks
    def _set_options(self, dtype):
        self._ctx.set_option("stage_device_f32", 0)

    def _prepare(self):
        """Pinned host slab + device slab instead of MDAnalysis' ``np.zeros`` position array."""
        super()._prepare()
        self.results.timeseries = None

    @staticmethod
    def _has_data(ts):
        return ts.has_positions

    def _evaluate(self):
        fft = bool(self.fft)
        self._run_kernels(functools.partial(self._ctx.msd, fft), lambda *a: self._ctx.msd_staged(fft, *a))
