"""Upper boundary of the hot path: the MDAnalysis ``AnalysisBase`` contract.

When MDAnalysis is importable the analysis classes subclass the real
``MDAnalysis.analysis.base.AnalysisBase`` and use its ``Results``,
``UpdatingAtomGroup``, ``NoDataError`` and ``units.constants``.  When it is not
(the build container and the GPU box have no MDAnalysis), the minimal
stand-ins below provide the same template-method protocol the reference relies
on (/root/reference/transport_analysis/velocityautocorr.py:120,142-206):
``run(start, stop, step, frames)`` -> ``_setup_frames`` -> ``_prepare`` ->
per frame ``_single_frame`` (with ``_frame_index``, ``_ts``, ``frames``,
``times`` maintained) -> ``_conclude`` -> ``self``.
"""
from __future__ import annotations

import warnings

import numpy as np

try:  # pragma: no cover - exercised only where MDAnalysis exists
    from MDAnalysis.analysis.base import AnalysisBase, Results
    from MDAnalysis.core.groups import UpdatingAtomGroup
    from MDAnalysis.exceptions import NoDataError
    from MDAnalysis.units import constants as _mda_constants

    HAVE_MDANALYSIS = True
    try:
        BOLTZMANN = _mda_constants["Boltzmann_constant"]
    except KeyError:  # MDAnalysis < 2.6 spelling (viscosity.py:138-142)
        BOLTZMANN = _mda_constants["Boltzman_constant"]
except ImportError:
    HAVE_MDANALYSIS = False
    #: kJ/(mol K); MDAnalysis.units.constants["Boltzmann_constant"]
    BOLTZMANN = 8.314462159e-3

    class NoDataError(ValueError):
        """Raised when a trajectory lacks data an analysis needs."""

    class UpdatingAtomGroup:  # only ever used for isinstance checks
        pass

    class Results(dict):
        """dict with attribute access, like MDAnalysis.analysis.base.Results."""

        def __getattr__(self, key):
            try:
                return self[key]
            except KeyError as err:
                raise AttributeError(f"'Results' object has no attribute '{key}'") from err

        def __setattr__(self, key, value):
            self[key] = value

        def __delattr__(self, key):
            try:
                del self[key]
            except KeyError as err:
                raise AttributeError(f"'Results' object has no attribute '{key}'") from err

    class AnalysisBase:
        """Serial frame loop with the hooks of MDAnalysis' AnalysisBase."""

        def __init__(self, trajectory, verbose=False, **kwargs):
            self._trajectory = trajectory
            self._verbose = verbose
            self.results = Results()

        def _setup_frames(self, trajectory, start=None, stop=None, step=None, frames=None):
            if frames is not None:
                if not all(opt is None for opt in (start, stop, step)):
                    raise ValueError("start/stop/step cannot be combined with frames")
                index = list(frames)
                self.start = self.stop = self.step = None
            else:
                n = len(trajectory)
                rng = range(*slice(start, stop, step).indices(n))
                index = list(rng)
                self.start, self.stop, self.step = rng.start, rng.stop, rng.step
            self._frame_indices = index
            self.n_frames = len(index)
            self.frames = np.zeros(self.n_frames, dtype=int)
            self.times = np.zeros(self.n_frames)

        def _prepare(self):
            pass

        def _single_frame(self):
            raise NotImplementedError

        def _conclude(self):
            pass

        def run(self, start=None, stop=None, step=None, frames=None, verbose=None, **kwargs):
            self._setup_frames(self._trajectory, start=start, stop=stop, step=step, frames=frames)
            self._prepare()
            for i, idx in enumerate(self._frame_indices):
                ts = self._trajectory[idx]
                self._frame_index = i
                self._ts = ts
                self.frames[i] = ts.frame
                self.times[i] = ts.time
                self._single_frame()
            self._conclude()
            return self


_DIM_KEYS = {
    "x": [0],
    "y": [1],
    "z": [2],
    "xy": [0, 1],
    "xz": [0, 2],
    "yz": [1, 2],
    "xyz": [0, 1, 2],
}


#: frames staged on the host before an asynchronous host->device copy is queued
_COMMIT_BYTES = 32 << 20


def parse_dim_type(dim_str, what="dim_type"):
    """Column indices and dimensionality factor for a (lower-cased) dim_type.

    Same table and error text as the reference
    (velocityautocorr.py:155-176, viscosity.py:144-165; MDAnalysis' EinsteinMSD with
    ``what="msd_type"``); order matters, so "yx" is invalid."""
    try:
        cols = _DIM_KEYS[dim_str]
    except KeyError:
        raise ValueError(
            "invalid {}: {} specified, please specify one of xyz, "
            "xy, xz, yz, x, y, z".format(what, dim_str)
        )
    return list(cols), len(cols)


def first_crossing(t, y, level):
    """The time at which the series y(t) first falls below ``level``, linearly interpolated between the two samples around
    the crossing (t[0] when y[0] is already below); NaN for a series that never does."""
    below = np.flatnonzero(y < level)
    if below.size == 0:
        return np.nan
    i = int(below[0])
    return t[0] if i == 0 else t[i - 1] + (level - y[i - 1]) * (t[i] - t[i - 1]) / (y[i] - y[i - 1])


def stage_columns(dst, src, lo, hi, dim):
    """dst[: hi - lo] = src[lo:hi][:, dim] (the reference's per-frame slab fill,
    velocityautocorr.py:192-194, viscosity.py:189-199) without the temporary the fancy index
    makes: every dim_type of the table is an arithmetic progression of columns, i.e. a slice
    (one strided copy straight into the pinned slab; 15x faster for "xyz" at 50000 atoms)."""
    n = hi - lo
    step = dim[1] - dim[0] if len(dim) > 1 else 1
    if step > 0 and all(b - a == step for a, b in zip(dim, dim[1:])):
        dst[:n] = src[lo:hi, dim[0]:dim[-1] + 1:step]
    else:  # not reachable from parse_dim_type's table
        dst[:n] = src[lo:hi][:, dim]


def native_rows(group):
    """How ta_stage_frame finds the group's atoms in a Timestep's arrays: (first atom, index array or None,
    count, largest index) from MDAnalysis' ``AtomGroup.ix`` (the stand-in's ``indices``); None when the
    group has neither or $TA_AMD_NATIVE_STAGING=0 (the frames are then staged through NumPy views)."""
    import os

    from . import _lib

    if os.environ.get("TA_AMD_NATIVE_STAGING", "1") == "0":
        return None
    ix = getattr(group, "ix", None)
    if ix is None:
        ix = getattr(group, "indices", None)
    if ix is None:
        return None
    ix = np.asarray(ix)
    if ix.ndim != 1 or ix.size == 0 or not np.issubdtype(ix.dtype, np.integer) or int(ix.min()) < 0:
        return None
    lo, index, n = _lib.atom_rows(ix)
    return (lo, index, n), int(ix.max())


def stage_frame_native(ctx, slab, frame, ts, attr, cols, rows):
    """slab[frame] = ts.<attr>[group's atoms][:, cols] in one native pass (ta_stage_frame: gather, column
    selection, conversion, on a few host threads, GIL released) -- what the reference's
    ``self.atomgroup.<attr>[:, self._dim]`` computes through two temporaries
    (velocityautocorr.py:192-194, viscosity.py:189-199).  False when the Timestep's array is not
    something the native call can read in place (the caller falls back to the NumPy path)."""
    from . import _lib

    if rows is None or not hasattr(ctx, "stage_frame"):
        return False
    try:
        arr = getattr(ts, attr)
    except Exception:
        return False
    src = _lib.frame_source(arr)
    if src is None or rows[1] >= arr.shape[0] or cols[-1] >= arr.shape[1]:
        return False
    ctx.stage_frame(slab, frame, src, cols, rows[0])
    return True


def pop_device_options(kwargs):
    """The placement keywords every analysis class takes, popped from its **kwargs:
    ``distributed`` (one process per GPU under torch.distributed), ``devices=[...]`` (several GPUs
    behind one object, exclusive with ``distributed``) and ``device`` (a GPU index or "cpu"; default
    the first of ``devices``, else this rank's device when distributed, else ``$TA_AMD_DEVICE`` or 0).
    Returns (distributed, devices or None, device index)."""
    import os

    from . import _lib

    distributed = bool(kwargs.pop("distributed", False))
    devices = kwargs.pop("devices", None)
    devices = None if devices is None else [int(d) for d in devices]
    if devices is not None and distributed:
        raise ValueError("devices=[...] (one process, several GPUs) and distributed=True "
                         "(one process per GPU) are exclusive")
    device = kwargs.pop("device", None)
    if device is None and devices:
        device = devices[0]
    if device is None:
        if distributed:  # one process per GPU: this rank's own device
            from .dist import default_device

            device = default_device()
        else:
            device = os.environ.get("TA_AMD_DEVICE", 0)
    return distributed, devices, _lib.device_index(device)


def open_context(devices, device):
    """The library handle of an analysis object: a ta_group for devices=[...], else one context."""
    from . import _lib

    return _lib.Group(devices) if devices is not None else _lib.Context(device)


class StagedAnalysis(AnalysisBase):
    """The run logic the analysis classes share: the frames' columns of ``_stage_arrays`` go into
    pinned host slabs (one per array, in that order) and on to the device during the frame loop,
    then ONE library call evaluates them.  The placement keywords (``device`` / ``devices`` /
    ``distributed``), ``by_particle`` and ``stage_dtype`` are handled here; under ``distributed=True``
    the lag sums are reduced over ranks, on the device when the process group is nccl (RCCL).

    A subclass sets ``self._group`` (the analysed AtomGroup), ``self.n_particles`` and ``self._dim`` /
    ``self.dim_fac``, names its by-particle result, gives the frame check of ``_has_data`` and
    implements ``_set_options`` (context options, set before the slabs are allocated) and
    ``_evaluate`` (one ``_run_kernels`` call with its host and staged entry points); its own keywords
    it pops in ``_pop_options``.  A subclass that stages ``positions`` may set ``self._unwrap``: the
    frame loop then records every frame's ``ts.dimensions`` and ``_conclude`` unwraps the position slab
    on the device (MDAnalysis' ``NoJump``, ``ta_unwrap``) after the last commit and before ``_evaluate``,
    on every placement (each rank or device member unwraps its own atoms: no communication).

    A subclass with ``_accepts_compound`` takes ``compound``, ``compound_weights`` and ``reference_frame`` and calls
    ``_init_compound()`` once ``self._group`` and ``self.n_particles`` are set: the frames are still staged (and unwrapped)
    as ATOMS, then ``_conclude`` replaces the slab by the slab of the compounds' weighted centres (``ta_compound``), and
    ``n_particles``, the by-particle result and every mean are those of the compounds.  A class without it leaves the three
    keywords to ``AnalysisBase``, which rejects them like any unknown keyword.

    No method here may take a name of MDAnalysis' ``AnalysisBase`` hooks: from 2.8 on its ``run()``
    calls ``self._compute(indexed_frames, ...)``, so ``_compute`` is theirs."""

    _stage_arrays = ()          # Timestep arrays staged, in slab order
    _by_particle_key = None     # results.<key>: the (n_frames, n_particles) array or None
    _no_data_message = None     # NoDataError text of a frame _has_data rejects
    _unwrap = False             # unwrap the staged positions (NoJump) before _evaluate
    _record_volumes = False     # record every frame's ts.volume; _evaluate finds their mean in self._vol_avg
    _accepts_compound = False   # takes compound / compound_weights / reference_frame (the subclass calls _init_compound)

    # MDAnalysis >= 2.8 parallel-analysis protocol: frames are staged into ONE device slab per
    # analysis object and every lag couples all frames, so a frame-split backend cannot apply;
    # the data-parallel axis of this path is atoms (distributed=True), not frames.
    _analysis_algorithm_is_parallelizable = False

    @classmethod
    def get_supported_backends(cls):
        return ("serial",)

    def __init__(self, group, **kwargs):
        self._want_by_particle = bool(kwargs.pop("by_particle", True))
        self._stage_dtype = kwargs.pop("stage_dtype", None)
        self._distributed, self._devices, self._device = pop_device_options(kwargs)
        self._plan = None  # (offsets, members, member weights, frame weights or None) of ta_compound
        if self._accepts_compound:
            # (compound_weights="mass", the default, asks for nothing by itself)
            given = [k for k in ("compound", "compound_weights", "reference_frame")
                     if kwargs.get(k) is not None and not (k == "compound_weights" and isinstance(kwargs[k], str) and kwargs[k] == "mass")]
            if given and (self._devices is not None or self._distributed):
                raise ValueError(f"{', '.join(given)}: not available with devices=[...] or distributed=True -- the atoms are "
                                 "split over the GPUs by index, and all atoms of a molecule would have to share a shard")
            self._compound = kwargs.pop("compound", None)
            self._compound_weights = kwargs.pop("compound_weights", "mass")
            self._reference_frame = kwargs.pop("reference_frame", None)
            if self._reference_frame not in (None, "barycentric"):
                raise ValueError(f"reference_frame: {self._reference_frame!r}, expected None or 'barycentric'")
        self._pop_options(kwargs)
        super().__init__(group.universe.trajectory, **kwargs)
        self._ctx = None

    def _pop_options(self, kwargs):
        """Pop (and check) the subclass's own keywords before AnalysisBase sees the rest."""

    def _group_attr(self, attr, what):
        try:
            return np.asarray(getattr(self._group, attr))
        except Exception as err:  # (MDAnalysis: NoDataError, an AttributeError subclass)
            raise ValueError(f"{what} needs the group's '{attr}', and it has none ({err})") from err

    def _init_compound(self):
        """The plan of ``ta_compound`` from the three keywords; ``n_particles`` becomes the number of compounds and
        ``_compound_index`` the compound of every atom.  Without ``compound`` and ``reference_frame`` nothing changes."""
        self._n_atoms = self.n_particles
        self.compound, self.reference_frame = self._compound, self._reference_frame
        if self._compound is None and self._reference_frame is None:
            return
        from .compound import COMPOUND_ATTRS, compound_plan

        n = self._n_atoms
        if self._compound is None:  # every atom its own compound: the frame of reference alone
            ids, offsets = np.arange(n), np.arange(n + 1, dtype=np.int64)
            members, weights = np.arange(n, dtype=np.int32), None
        else:
            if isinstance(self._compound, str):
                if self._compound not in COMPOUND_ATTRS:
                    raise ValueError(f"compound: {self._compound!r}, expected one of {sorted(COMPOUND_ATTRS)} or one integer "
                                     "label per atom")
                labels = self._group_attr(COMPOUND_ATTRS[self._compound], f"compound={self._compound!r}")
            else:
                labels = np.asarray(self._compound)
                if labels.ndim != 1 or labels.size != n or not np.issubdtype(labels.dtype, np.integer):
                    raise ValueError(f"compound: one integer label per atom is expected ({n} atoms), got an array of shape "
                                     f"{labels.shape} and dtype {labels.dtype}")
            cw = self._compound_weights
            if isinstance(cw, str):
                if cw not in ("mass", "geometry"):
                    raise ValueError(f"compound_weights: {cw!r}, expected 'mass', 'geometry' or one value per atom")
                per_atom = self._group_attr("masses", "compound_weights='mass'") if cw == "mass" else np.ones(n)
            else:
                per_atom = np.asarray(cw, dtype=np.float64).ravel()
            ids, offsets, members, weights = compound_plan(labels, per_atom)
        frame = None
        if self._reference_frame == "barycentric":
            m = self._group_attr("masses", "reference_frame='barycentric'").astype(np.float64)
            if m.size != n or not m.sum() > 0:
                raise ValueError("reference_frame='barycentric' needs masses with a positive sum, one per atom")
            frame = m / m.sum()
        self._plan = (offsets, members, weights, frame)
        self._compound_ids = ids
        self._compound_index = np.empty(n, dtype=np.int64)
        self._compound_index[members] = np.repeat(np.arange(ids.size), np.diff(offsets))
        self.n_particles = int(ids.size)

    def _pick_stage_dtype(self):
        """float32 when the trajectory hands out every staged array in float32 (MDAnalysis does):
        lossless, half the PCIe bytes of the reference's float64 slab; the arithmetic is float64."""
        if self._stage_dtype is not None:
            return np.dtype(self._stage_dtype)
        try:
            f32 = all(np.asarray(getattr(self._group, a)).dtype == np.float32 for a in self._stage_arrays)
        except Exception:  # missing data: _single_frame raises NoDataError, as the reference does
            return np.dtype(np.float64)
        return np.dtype(np.float32) if f32 else np.dtype(np.float64)

    def _prepare(self):
        """Pinned host slabs + device slabs instead of the reference's ``np.zeros`` arrays."""
        if self._ctx is None:
            self._ctx = open_context(self._devices, self._device)
        # staging is sized by the atoms, everything after ta_compound by the compounds (n_particles)
        n_stage = self._n_atoms if self._plan is not None else self.n_particles
        self._lo, self._hi = 0, n_stage
        self._source = self._group  # whose arrays a frame is read from
        self._rccl = False  # the lag sums stay on the GPU through the reduce
        if self._distributed:
            from .dist import check_backend, shard_of_this_rank, uses_device_reduce

            _, _, self._lo, self._hi = shard_of_this_rank(self.n_particles)
            check_backend(self._device, 'device="cpu"')
            self.results.particle_range = (self._lo, self._hi)
            # this rank's block only: the trajectory gathers hi - lo atoms per frame, not all of them
            self._source = self._group[self._lo:self._hi]
            self._rccl = uses_device_reduce()
        self._n_local = self._hi - self._lo
        dtype = self._pick_stage_dtype()
        self._set_options(dtype)
        n_slabs = len(self._stage_arrays)
        if self._devices is not None:
            # one pinned slab per array and GPU, each holding that GPU's column block; filled in ONE frame loop
            slabs = self._ctx.stage_alloc(self.n_frames, self.n_particles, self.dim_fac, n_slabs=n_slabs, dtype=dtype)
            self._targets = [(views, lo, hi) for *views, (lo, hi) in zip(*slabs, self._ctx.shards) if hi > lo]
            self.results.device_ranges = list(self._ctx.shards)
        else:
            slabs = self._ctx.stage_alloc(self.n_frames, max(self._n_local, 1), self.dim_fac, n_slabs=n_slabs,
                                          dtype=dtype)
            # columns of the source group: the distributed source is the block itself
            self._targets = [(slabs, 0, self._n_local)]
        for attr, slab in zip(self._stage_arrays, slabs):
            setattr(self, "_" + attr, slab)
        self._fills = tuple(enumerate(self._stage_arrays))  # (slab, Timestep array) pairs of the frame loop
        # the per-frame fill reads the Timestep's own arrays natively (ta_stage_frame) where it can
        self._rows = native_rows(self._source) if self._n_local else None
        frame_bytes = max(1, n_slabs * self._n_local * self.dim_fac * dtype.itemsize)
        self._commit_every = max(1, _COMMIT_BYTES // frame_bytes)
        self._committed = 0
        if self._by_particle_key is not None:
            setattr(self.results, self._by_particle_key, None)
        # the (n_frames, n_particles) result array lives in pinned host memory, page-locked on a
        # helper thread while the frames are staged
        # unwrap: the box of every analysed frame, (n_frames, 6) = ts.dimensions
        self._boxes = np.zeros((self.n_frames, 6)) if self._unwrap else None
        self._volumes = np.zeros(self.n_frames) if self._record_volumes else None
        self._bp_home = None
        if self._want_by_particle and self._n_local and not self._rccl:
            n_out = self.n_particles if self._plan is not None else self._n_local
            self._bp_home = self._ctx.result_home((self.n_frames, n_out))
        if self._plan is not None:
            self.results.compound_ids = self._compound_ids

    def _single_frame(self):
        """Stage the selected columns of one frame's arrays."""
        ts = self._ts
        if not self._has_data(ts):
            raise NoDataError(self._no_data_message)
        i = self._frame_index
        if self._boxes is not None:
            self._boxes[i] = self._unwrap_box(ts)
        if self._volumes is not None:
            self._volumes[i] = ts.volume
        if self._n_local:
            for slab, attr in self._fills:
                if not stage_frame_native(self._ctx, slab, i, ts, attr, self._dim, self._rows):
                    src = np.asarray(getattr(self._source, attr))
                    for views, lo, hi in self._targets:
                        stage_columns(views[slab][i], src, lo, hi, self._dim)
        if i + 1 - self._committed >= self._commit_every:
            self._ctx.stage_commit(self._committed, i + 1)
            self._committed = i + 1

    def _unwrap_box(self, ts):
        """ts.dimensions as unwrapping needs it, or the ValueError of a box it cannot use."""
        dims = ts.dimensions
        if dims is None:
            raise ValueError(f"unwrap=True needs the periodic box, and frame {ts.frame} has none (ts.dimensions is None)")
        d = np.asarray(dims, dtype=np.float64).ravel()
        if d.shape != (6,) or not np.all(np.isfinite(d)) or not np.all(d[:3] > 0):
            raise ValueError(f"unwrap=True needs box lengths > 0: frame {ts.frame} has dimensions {list(d)}")
        if self.dim_fac != 3 and not np.all(d[3:] == 90.0):
            raise ValueError(f"unwrap=True with a non-orthogonal box (frame {ts.frame}: angles {list(d[3:])}) needs "
                             "all three dimensions ('xyz'): a triclinic image shift mixes the axes")
        return d

    def _conclude(self):
        if self._committed < self.n_frames:
            self._ctx.stage_commit(self._committed, self.n_frames)
            self._committed = self.n_frames
        if self._boxes is not None:
            frames = np.asarray(self.frames)
            if frames.size > 1 and np.any(np.diff(frames) != 1):
                warnings.warn("unwrap=True over frames that are not consecutive (step > 1 or a frames= list): the "
                              "positions are unwrapped over the analysed frames only, and a particle that moves more "
                              "than half a box between two of them is not unwrapped correctly", UserWarning,
                              stacklevel=3)
            if self._n_local or self._devices is not None:
                self._ctx.unwrap(self._stage_arrays.index("positions"), self._boxes, self._dim)
        if self._volumes is not None:
            self._vol_avg = np.average(self._volumes)
        if self._plan is not None:  # after the unwrap, which must see atoms: molecules from here on
            self._ctx.compound(*self._plan)
        self._evaluate()

    def _run_kernels(self, host, launch):
        """results.timeseries and the by-particle result of the staged slabs.  host(by_particle=, out=)
        -> (timeseries, by-particle or None) is the library call; launch(d_lagsum, d_bp, ld_bp, stream)
        its staged twin, which only the RCCL path calls (see dist.staged_timeseries_on_device) -- so it
        looks the context's ``*_staged`` method up when called: a device group has none."""
        if self._rccl:
            from .dist import staged_timeseries_on_device

            ts, bp = staged_timeseries_on_device(launch, self.n_frames, self._n_local, self.n_particles,
                                                 self._device, by_particle=self._want_by_particle)
        else:
            home = self._bp_home.get() if self._bp_home is not None else None
            self._bp_home = None
            ts, bp = host(by_particle=self._want_by_particle, out=home)
            if self._distributed:
                from .dist import allreduce_mean_over_atoms

                if self._n_local == 0:  # more ranks than atoms: this rank contributes nothing
                    ts, bp = np.zeros(self.n_frames), (None if bp is None else bp[:, :0])
                ts = allreduce_mean_over_atoms(ts, self._n_local, self.n_particles, self._device)
        setattr(self.results, self._by_particle_key, bp)
        self.results.timeseries = ts


class CollectiveAnalysis(StagedAnalysis):
    """What the collective analyses share: the Einstein-Helfand ones (``ConductivityHelfand``, ``OnsagerHelfand``) and their
    Green-Kubo twins (``greenkubo.py``: the sums are currents of the staged velocities, ``_stage_arrays``, ``_has_data``
    and ``_set_options`` overridden).  Their quantity is
    the mean squared displacement of sums over all atoms -- the moments -- and not a mean of per-particle series: there
    is no by-particle result, and under ``distributed=True`` every rank forms the moments of its block of atoms, the
    moments are summed over ranks, and ONE correlation of the sums follows (the MSD of a sum is not the sum of the MSDs).

    A subclass gives the wording of the two refusals, pops nothing of its own, and implements ``_moments(fft, lo, hi,
    correlate)`` (one library call on the atoms [lo, hi) -> (tuple of the arrays that add up over atoms, None for one
    not asked for; their correlation or None)), ``_no_moments()`` (that tuple as zeros: a rank without atoms),
    ``_correlate(fft, sums)`` (the correlation of summed moments) and ``_store(sums, correlation)`` (results and fit)."""

    _stage_arrays = ("positions",)
    _record_volumes = True
    _updating_message = None     # TypeError text for an UpdatingAtomGroup
    _by_particle_message = None  # TypeError text for by_particle=True

    def __init__(self, atomgroup, temp_avg, dim_type, linear_fit_window, fft, unwrap, kwargs):
        if isinstance(atomgroup, UpdatingAtomGroup):
            raise TypeError(self._updating_message)
        if kwargs.pop("by_particle", False):
            raise TypeError(self._by_particle_message)
        super().__init__(atomgroup, by_particle=False, **kwargs)
        self._unwrap = self.unwrap = bool(unwrap)
        self.temp_avg = temp_avg
        self.dim_type = dim_type.lower()
        self._dim, self.dim_fac = parse_dim_type(self.dim_type)
        self.linear_fit_window = linear_fit_window
        self.fft = fft
        self.atomgroup = self._group = atomgroup
        self.n_particles = len(self.atomgroup)
        if self._accepts_compound:
            self._init_compound()

    def _per_atom(self, values, name, unit, dtype=np.float64):
        """One value per atom of the group (with ``compound``: per compound) as a flat array, or the ValueError that says
        how many there are."""
        a = np.asarray(values, dtype=dtype).ravel()
        if a.size != self.n_particles:
            what = "atoms" if self._plan is None or self._compound is None else "compounds"
            raise ValueError(f"{name}: {a.size} {unit} for {self.n_particles} {what}")
        return a

    def _species_labels(self, species):
        """One species label per particle: with ``compound`` one per compound, or one per atom that is the same within
        every compound (``species="resnames"``)."""
        # a topology attribute, or a subclass's own per-atom labels: certainly one label per atom
        named = isinstance(species, str) or getattr(self, "_species_per_atom", False)
        if isinstance(species, str):
            species = getattr(self.atomgroup, species)
        if self._plan is not None and self._compound is not None:
            from .compound import per_compound

            return per_compound(species, self._compound_index, self.n_particles, "species", per_atom=True if named else None)
        return self._per_atom(species, "species", "labels", dtype=None)

    def _set_options(self, dtype):
        self._ctx.set_option("stage_device_f32", 0)

    @staticmethod
    def _has_data(ts):
        return ts.has_positions and ts.volume != 0

    def _evaluate(self):
        fft = bool(self.fft)
        if self._distributed:
            from .dist import allreduce_sum

            # (more ranks than atoms: a rank without atoms contributes zeros)
            sums = self._moments(fft, self._lo, self._hi, False)[0] if self._n_local else self._no_moments()
            sums = tuple(None if a is None else allreduce_sum(a, self._device) for a in sums)
            correlation = self._correlate(fft, sums)
        else:
            sums, correlation = self._moments(fft, 0, self.n_particles, True)
        self._store(sums, correlation)

    def lag_times(self):
        """Lag times k * dt (ps) of the timeseries, dt the spacing of the analysed frames' times."""
        dt = float(self.times[1] - self.times[0]) if self.n_frames > 1 else 0.0
        return np.arange(self.n_frames) * dt

    def _slope(self, series):
        """Slope of a lag-indexed series against lag time over the lag indices [lo, hi) of ``linear_fit_window``."""
        lo, hi = self.linear_fit_window[0], self.linear_fit_window[1]
        return np.polyfit(self.lag_times()[lo:hi], series[lo:hi], 1)[0]
