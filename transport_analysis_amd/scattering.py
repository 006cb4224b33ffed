"""Intermediate scattering functions F_s(k, t) and F(k, t) on MI355X, from positions.

    F_s(k, t) = 1/N < sum_n exp(i k . (x_n(t0 + t) - x_n(t0))) >        (self, incoherent)
    F(k, t)   = 1/N < rho_k(t0 + t) rho_k(t0)* >,   rho_k(t) = sum_n exp(i k . x_n(t))        (collective, coherent)

averaged over time origins t0.  ``exp(i k . x_n(t))`` is one complex series per atom and wavevector: one pass over the
position slab (``k_phase`` behind ``ta_scatter`` of ``include/ta_hip.h``, hand-written HIP; a float32 slab is read as
float32, never widened first) writes it as a slab of (cos, sin) column pairs, on which the library's VACF lag sums give
the self part and its species-sum pass the density.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from ._base import CollectiveAnalysis, first_crossing, parse_dim_type


def triclinic_vectors(dimensions):
    """The (3, 3) box matrix (rows a, b, c) of [a, b, c, alpha, beta, gamma] (degrees), a along x and b in the xy plane:
    MDAnalysis' ``lib.mdamath.triclinic_vectors`` in float64."""
    d = np.asarray(dimensions, dtype=np.float64).ravel()
    if d.shape != (6,) or not np.all(np.isfinite(d)) or not np.all(d[:3] > 0):
        raise ValueError(f"a box with lengths > 0 is needed, got dimensions {list(d)}")
    a, b, c = d[:3]
    if np.all(d[3:] == 90.0):
        return np.diag([a, b, c])
    ca, cb, cg = (0.0 if x == 90.0 else np.cos(np.deg2rad(x)) for x in d[3:])
    sg = 1.0 if d[5] == 90.0 else np.sin(np.deg2rad(d[5]))
    H = np.zeros((3, 3))
    H[0, 0] = a
    H[1, 0], H[1, 1] = b * cg, b * sg
    H[2, 0] = c * cb
    H[2, 1] = c * (ca - cb * cg) / sg
    z2 = c * c - H[2, 0] ** 2 - H[2, 1] ** 2
    if not z2 > 0:
        raise ValueError(f"the box angles {list(d[3:])} do not span a volume")
    H[2, 2] = np.sqrt(z2)
    return H


def kvectors_from_box(dimensions, q, dq, max_vectors=32, dim_type="xyz"):
    """Wavevectors commensurate with a periodic box, by magnitude shell.

    ``dimensions``: [a, b, c, alpha, beta, gamma]; ``q``: a scalar or a sequence of magnitudes (rad per length unit),
    ``dq``: the full width of every shell, ``|k|`` in [q - dq / 2, q + dq / 2].  The integer triples m with zeros outside
    the box axes of ``dim_type`` are enumerated, k = 2 pi m H^-1T with H the box matrix (``triclinic_vectors``;
    orthorhombic and triclinic boxes).  Of each pair +k, -k the one whose first non-zero m is positive is kept; a shell's
    vectors are sorted by (|m|^2, m lexicographic) and the first ``max_vectors`` kept.  An empty shell: ``ValueError``.

    Returns (kvectors (K, dim) -- the components of ``dim_type``, shell (K,) -- the index into ``q`` of every vector).
    With a non-orthogonal box every vector has components along all three axes: ``dim_type`` must then be "xyz"."""
    cols, _ = parse_dim_type(str(dim_type).lower())
    H = triclinic_vectors(dimensions)
    ortho = bool(np.all(H == np.diag(np.diag(H))))
    if not ortho and len(cols) != 3:
        raise ValueError("a non-orthogonal box needs dim_type='xyz': its reciprocal vectors mix the axes")
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64)).ravel()
    dq = float(dq)
    max_vectors = int(max_vectors)
    if qs.size < 1 or not np.all(np.isfinite(qs)) or not np.all(qs > 0) or not dq > 0 or max_vectors < 1:
        raise ValueError("q must be positive magnitudes, dq > 0 and max_vectors >= 1")
    B = 2.0 * np.pi * np.linalg.inv(H)  # columns: the reciprocal vectors; k = m @ B.T
    q_hi = float(qs.max()) + 0.5 * dq
    # |m_i| <= |k| |row i of H| / (2 pi): m = H k / (2 pi)
    m_max = np.floor(q_hi * np.linalg.norm(H, axis=1) / (2.0 * np.pi) + 1e-9).astype(np.int64)
    m_max = np.where(np.isin(np.arange(3), cols), m_max, 0)
    if np.prod(2.0 * m_max + 1.0) > 5e7:
        raise ValueError(f"q + dq / 2 = {q_hi} spans {int(np.prod(2.0 * m_max + 1.0))} lattice points of this box: too many")
    grids = np.meshgrid(*[np.arange(-n, n + 1) for n in m_max], indexing="ij")
    m = np.stack([g.ravel() for g in grids], axis=1)
    # one of each +-k pair: the first non-zero component positive (and not m = 0)
    first = np.where(m[:, 0] != 0, m[:, 0], np.where(m[:, 1] != 0, m[:, 1], m[:, 2]))
    m = m[first > 0]
    k = m @ B.T
    kn = np.linalg.norm(k, axis=1)
    m2 = (m * m).sum(axis=1)
    vecs, shells = [], []
    for s, q0 in enumerate(qs):
        sel = np.flatnonzero((kn >= q0 - 0.5 * dq) & (kn <= q0 + 0.5 * dq))
        if sel.size == 0:
            raise ValueError(f"no wavevector of this box has a magnitude within {0.5 * dq} of q = {q0}: widen dq")
        order = np.lexsort((m[sel, 2], m[sel, 1], m[sel, 0], m2[sel]))
        sel = sel[order][:max_vectors]
        vecs.append(k[sel][:, cols])
        shells.append(np.full(sel.size, s, dtype=np.int64))
    return np.ascontiguousarray(np.concatenate(vecs)), np.concatenate(shells)


def explicit_kvectors(kvectors, dim_fac, dim_type):
    """Explicit wavevectors as a C-contiguous float64 (K, dim_fac) array, or the ValueError that says what is wrong."""
    k = np.ascontiguousarray(kvectors, dtype=np.float64)
    if k.ndim != 2 or k.shape[0] < 1 or k.shape[1] != dim_fac:
        raise ValueError(f"kvectors: shape {k.shape}, expected (K, {dim_fac}) for dim_type={dim_type!r}")
    if not np.all(np.isfinite(k)):
        raise ValueError("kvectors must be finite")
    return k


def shell_mean(shell, by_kvector):
    """(n_frames, n_shells): the mean of a (n_frames, K) array over the vectors of every shell"""
    n_shells = int(shell.max()) + 1
    counts = np.bincount(shell, minlength=n_shells)
    out = np.zeros((by_kvector.shape[0], n_shells))
    np.add.at(out.T, shell, by_kvector.T)
    return out / counts


class BoxWavevectors:
    """What the k-space classes share: ``kvectors`` used as they are or, with ``q`` / ``dq`` / ``max_vectors``,
    ``kvectors_from_box`` of the first analysed frame's box, and the shell means.  The class sets ``q``, ``dq``,
    ``max_vectors``, ``kvectors`` and ``shell`` (``_init_kvectors``) and calls ``_box_kvectors()`` at the top of
    ``_single_frame``."""

    def _init_kvectors(self, kvectors, q, dq, max_vectors):
        if (kvectors is None) == (q is None):
            raise ValueError("exactly one of kvectors (explicit wavevectors) and q (magnitudes, with dq) must be given")
        if kvectors is None and dq is None:
            raise ValueError("q needs the shell width dq")
        self.q, self.dq, self.max_vectors = q, dq, int(max_vectors)
        self.kvectors = self.shell = None
        if kvectors is not None:
            self.kvectors = explicit_kvectors(kvectors, self.dim_fac, self.dim_type)

    def _box_kvectors(self):
        if self.q is not None and self._frame_index == 0:
            dims = self._ts.dimensions
            if dims is None:
                raise ValueError("q= needs the periodic box of the first analysed frame, and it has none: give kvectors")
            self.kvectors, self.shell = kvectors_from_box(dims, self.q, self.dq, self.max_vectors, self.dim_type)

    def _shell_mean(self, by_kvector):
        return shell_mean(self.shell, by_kvector)


class IntermediateScattering(BoxWavevectors, CollectiveAnalysis):
    r"""Self and collective intermediate scattering functions of a group of atoms (or of molecules' centres).

    .. math:: F_s(\mathbf{k}, \tau) = \frac{1}{N} \frac{1}{T - \tau} \sum_{t < T - \tau} \sum_n
              \cos \mathbf{k} \cdot (\mathbf{x}_n(t + \tau) - \mathbf{x}_n(t)), \qquad
              F(\mathbf{k}, \tau) = \frac{1}{N} \frac{1}{T - \tau} \sum_{t < T - \tau} \mathrm{Re}\,
              \rho_\mathbf{k}(t + \tau) \rho_\mathbf{k}(t)^*

    Parameters
    ----------
    atomgroup : AtomGroup — the trajectory must hold positions.
    kvectors : (K, D) array in rad/A, used as they are (one component per dimension of ``dim_type``), or None.
    q, dq, max_vectors : keyword-only — instead of ``kvectors``: magnitudes (a scalar or a sequence, rad/A) and the shell
        width; the vectors are ``kvectors_from_box`` of the first analysed frame's box, at most ``max_vectors`` per shell.
        Exactly one of ``kvectors`` and ``q`` must be given.
    dim_type : {'xyz', 'xy', 'yz', 'xz', 'x', 'y', 'z'}
    fft : bool — ``True``: ``VelocityAutocorr``'s FFT evaluation for the correlations; ``False``: the direct forms.
    coherent : bool, default True — also the density and the collective function.
    unwrap : bool, default False — undo periodic wrapping first (``EinsteinMSD``'s).  Wavevectors commensurate with a
        constant box (``q=``) give phases that are invariant under wrapping: wrapped positions need no unwrapping.
    compound, compound_weights, reference_frame : keyword-only — as for ``EinsteinMSD``: the functions of molecules'
        centres; N is then the number of compounds.
    device, devices, distributed, stage_dtype : keyword-only — as for the other classes.  float32 staging stays float32
        on the device (unless ``unwrap=True``, which works on float64 slabs): the phase pass reads it as it is.  Under
        ``distributed=True`` and ``devices=[...]`` the self parts and densities of the blocks of atoms are summed
        BEFORE the collective correlation.
    A box is not needed with explicit ``kvectors``.  ``by_particle=True`` raises ``TypeError``.

    Attributes
    ----------
    results.kvectors (K, D); results.shell (K,) the shell of every vector (explicit ``kvectors``: each its own);
    results.q_shell (n_shells,) the mean \|k\| per shell; results.fs_by_kvector (n_frames, K); results.fs (n_frames,
    n_shells) the shell mean; with ``coherent``: results.density (K, n_frames, 2) = (Re, Im) rho_k(t), results.f_by_kvector
    (n_frames, K), results.f (n_frames, n_shells) and results.sk (n_shells,) = f[0], the static structure factor.
    """

    _accepts_compound = True
    _record_volumes = False
    _no_data_message = "Intermediate scattering function computation requires positions in the trajectory"
    _updating_message = "UpdatingAtomGroups are not valid for intermediate scattering function computation"
    _by_particle_message = ("IntermediateScattering has no per-particle result: the functions are sums over all atoms "
                            "(by_particle=True is not supported)")

    def __init__(self, atomgroup, kvectors=None, *, q=None, dq=None, max_vectors=32, dim_type="xyz", fft=True,
                 coherent=True, unwrap=False, **kwargs):
        super().__init__(atomgroup, None, dim_type, None, fft, unwrap, kwargs)
        self.coherent = bool(coherent)
        self._init_kvectors(kvectors, q, dq, max_vectors)
        if self.kvectors is not None:
            self.shell = np.arange(self.kvectors.shape[0])

    def _set_options(self, dtype):
        # float32 staging stays float32 on the device: k_phase reads it as it is (the unwrap pass works on float64 slabs)
        self._ctx.set_option("stage_device_f32", int(dtype == np.float32 and not self._unwrap))

    @staticmethod
    def _has_data(ts):
        return ts.has_positions

    def _prepare(self):
        super()._prepare()
        for key in ("kvectors", "shell", "q_shell", "fs_by_kvector", "fs", "density", "f_by_kvector", "f", "sk"):
            setattr(self.results, key, None)

    def _single_frame(self):
        self._box_kvectors()
        super()._single_frame()

    def _moments(self, fft, lo, hi, correlate):
        fs, rho, coll = self._ctx.scatter(fft, self.kvectors, density=self.coherent, collective=self.coherent and correlate)
        return (fs, rho), coll

    def _no_moments(self):
        K = self.kvectors.shape[0]
        return (np.zeros((K, self.n_frames)), np.zeros((K, self.n_frames, 2)) if self.coherent else None)

    def _correlate(self, fft, sums):
        return self._ctx.scatter_collective(sums[1], fft) if self.coherent else None

    def _store(self, sums, coll):
        N = float(self.n_particles)
        r = self.results
        r.kvectors, r.shell = self.kvectors, self.shell
        norms = np.linalg.norm(self.kvectors, axis=1)
        r.q_shell = np.bincount(self.shell, weights=norms) / np.bincount(self.shell)
        r.fs_by_kvector = np.ascontiguousarray(sums[0].T) / N
        r.fs = self._shell_mean(r.fs_by_kvector)
        if self.coherent:
            r.density = sums[1]
            r.f_by_kvector = np.ascontiguousarray(coll.T) / N
            r.f = self._shell_mean(r.f_by_kvector)
            r.sk = r.f[0].copy()

    def relaxation_times(self, level=1.0 / np.e):
        """(n_shells,) lag time (ps) at which ``fs / fs[0]`` first falls below ``level``, linearly interpolated between the
        two lags around the crossing; NaN for a shell that never does."""
        if self.results.get("fs") is None:
            raise RuntimeError("Analysis must be run prior to reading relaxation times")
        t = self.lag_times()
        fs = self.results.fs
        return np.array([first_crossing(t, fs[:, s] / fs[0, s], level) for s in range(fs.shape[1])])
