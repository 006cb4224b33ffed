"""Reorientation of molecules WHILE they stay in the solvation shell of a group on MI355X, from positions: the shell-resolved
rotational correlation functions C_1 and C_2 of molecule-fixed unit vectors (MDAnalysis' ``waterdynamics``
``WaterOrientationalRelaxation`` for a selection zone; the retardation factors of water around a solute, an ion or a surface).
``ShellResidence`` answers how long a molecule stays in the shell and ``ShellMSD`` how fast it moves there; this class answers
how fast it turns.  The indicator g(t) is ``ShellResidence``'s of the vector's ANCHOR atom, bit for bit, formed by the same
passes; one more kernel (``k_shell_orient`` behind ``ta_shell_orient`` of ``include/ta_hip.h``, hand-written HIP, the second
instantiation of ``k_shell_msd``'s gated walk) forms the unit vectors where they are needed and adds up u(t) . u(t + tau) and
its square over the lags 0 ... ``max_lag``; no block of unit vectors is ever written.  ``device="cpu"`` runs the opt-in CPU
backend's twin (the same arithmetic); a GPU context never falls back to it.
"""
from __future__ import annotations

import numpy as np

from ._lib import ORIENT_MODES
from .pair_lifetime import _trapezoid
from .shell_residence import _GatedShell


class ShellOrientation(_GatedShell):
    r"""C_1 and C_2 of molecule-fixed unit vectors while their molecule is in the shell of a reference group.

    .. math:: C_1(\tau) = \frac{\sum_n \sum_{t < T - \tau} w_n(t, \tau)\, c}{N(\tau)}, \qquad
              C_2(\tau) = \frac{1}{2} \Big( 3 \frac{\sum_n \sum_{t < T - \tau} w_n(t, \tau)\, c^2}{N(\tau)} - 1 \Big),
              \qquad c = \mathbf{u}_n(t) \cdot \mathbf{u}_n(t + \tau), \quad N(\tau) = \sum_n \sum_{t < T - \tau} w_n(t, \tau)

    with :math:`w = \prod_{s = t}^{t + \tau} g_n(s)` for ``condition="continuous"`` and :math:`w = g_n(t) g_n(t + \tau)` for
    ``condition="endpoints"``; g_n is ``ShellResidence``'s indicator of the vector's anchor atom after ``r_break`` and
    ``intermittency``.  ``condition="endpoints"`` is ``WaterOrientationalRelaxation``'s selection: the molecules present at both
    ends of the interval, whatever happened between.

    Each function is a RATIO OF SUMS over all time origins.  MDAnalysis averages the per-origin means instead; the two agree
    when the number of molecules inside is constant, and differ otherwise (origins with many molecules inside weigh more here).
    The per-origin form is not computed.

    The unit vectors are ``OrientationalCorrelation``'s (``mode``: ``"bond"`` a -> b, ``"bisector"`` d(a -> b) + d(a -> c),
    ``"normal"`` their cross product).  With ``periodic=True`` the frames' boxes serve the distance pass and the vectors' image
    step, so molecules that the trajectory wraps across a face need no unwrapping.  A degenerate vector (zero length) adds zeros
    to the sums and IS counted in N, because the gate is the shell alone; ``count[0] * c1[0]`` is the number of non-degenerate
    terms at lag 0.

    Parameters
    ----------
    reference : AtomGroup — the group whose shell is meant.
    atomgroup : AtomGroup — the atoms of the molecules that are followed; the union with ``reference`` is staged once.
    vectors : (N, 2) for ``mode="bond"``, else (N, 3), integers — positions WITHIN ``atomgroup``, one row per vector.
    mode : keyword-only, ``"bond"`` (default), ``"bisector"`` or ``"normal"``.
    anchor : keyword-only, default 0 — the column of ``vectors`` whose atom is in or out of the shell.  The observed atoms are
        ``atomgroup[vectors[:, anchor]]``; they must be distinct (two vectors on one anchor, OH1 and OH2 of a water, are two
        analyses whose sums and counts add), and the same set as ``reference`` or disjoint from it.  The other atoms of a row
        may belong to either group.
    r_cut, r_break, intermittency, periodic, device, stage_dtype : as for ``ShellResidence``.
    max_lag, condition : keyword-only, as for ``ShellMSD``.
    dim_type : only ``"xyz"``.

    ``fft=``, ``compound``, ``reference_frame``, ``unwrap`` and ``by_particle=True`` raise ``TypeError``; ``devices=[...]`` with
    more than one member and ``distributed=True`` raise ``ValueError``.

    Attributes
    ----------
    results.times (L + 1,) ps; results.count (L + 1,) int64 the terms N(tau); results.c1, results.c2 (L + 1,), ``nan`` where
    count is 0; results.n_inside, results.mean_inside, results.run_lengths as ``ShellResidence``'s; results.survival = ``count /
    n0`` as ``ShellMSD``'s; results.tau_1, results.tau_2 the trapezoid integrals of c1, c2 over times.  Where no anchor is ever
    inside: ``nan`` (a warning).
    """

    _no_data_message = "Shell orientation computation requires positions in the trajectory"
    _updating_message = "UpdatingAtomGroups are not valid for shell orientation computation"
    _by_particle_message = ("ShellOrientation has no per-particle result: the sums run over all vectors "
                            "(by_particle=True is not supported)")
    _result_keys = ("times", "count", "c1", "c2", "n_inside", "mean_inside", "run_lengths", "survival", "tau_1", "tau_2")
    _nothing_inside = "no anchor atom is inside the shell in any frame; the correlation functions are nan"

    def __init__(self, reference, atomgroup, vectors, *, mode="bond", anchor=0, r_cut, r_break=None, intermittency=0, max_lag=None,
                 condition="continuous", periodic=True, dim_type="xyz", **kwargs):
        self._refuse_fft(kwargs)
        if dim_type != "xyz":
            raise ValueError(f"ShellOrientation needs dim_type='xyz' (a unit vector has three components), got {dim_type!r}")
        self._check_condition(condition)
        if mode not in ORIENT_MODES:
            raise ValueError(f"mode: {mode!r}, expected one of {sorted(ORIENT_MODES)}")
        max_lag = self._check_max_lag(max_lag)
        width = 2 if mode == "bond" else 3
        if int(anchor) != anchor or not 0 <= anchor < width:
            raise ValueError(f"anchor must be a column of vectors, 0 ... {width - 1}, got {anchor}")
        own = np.asarray(atomgroup.ix if hasattr(atomgroup, "ix") else atomgroup.indices, dtype=np.int64)
        v = np.asarray(vectors)
        if v.ndim != 2 or v.shape[0] < 1 or v.shape[1] != width or not np.issubdtype(v.dtype, np.integer):
            raise ValueError(f"vectors: shape {v.shape} and dtype {v.dtype}, expected an integer (N, {width}) array of positions "
                             f"within the group for mode={mode!r}")
        if v.min() < 0 or v.max() >= own.size:
            raise ValueError(f"vectors: entries must be positions within the group, 0 ... {own.size - 1}")
        atoms = own[v]  # universe indices
        s = np.sort(atoms, axis=1)
        if np.any(s[:, 1:] == s[:, :-1]):
            raise ValueError(f"vectors: row {int(np.flatnonzero(np.any(s[:, 1:] == s[:, :-1], axis=1))[0])} names an atom twice")
        if np.unique(atoms[:, anchor]).size != atoms.shape[0]:
            raise ValueError("vectors: two rows share an anchor atom; the observed atoms must be distinct (analyse the second "
                             "vector of a molecule in a run of its own: the sums and counts add)")
        self._staged_with = np.unique(atoms)
        super().__init__(reference, atomgroup[v[:, anchor]], r_cut=r_cut, r_break=r_break, intermittency=intermittency, periodic=periodic,
                         fft=False, dim_type=dim_type, **kwargs)
        self.mode, self.anchor, self.max_lag, self.condition = mode, int(anchor), max_lag, condition
        self.n_vectors = int(atoms.shape[0])
        # the rows as staged items, in the order of their anchors: row n belongs to observed item n
        rows = np.searchsorted(self._union, atoms)
        self.vectors = np.ascontiguousarray(rows[np.argsort(rows[:, self.anchor], kind="stable")], dtype=np.int32)

    def _moments(self, fft, lo, hi, correlate):
        all_a = self.n_a == self.n_particles
        out = self._ctx.shell_orient(self.condition, self._max_lag, self.vectors, self.mode, self.r_cut, anchor=self.anchor,
                                     r_break=self.r_break, gap=self.intermittency, idx_a=None if all_a else self._idx_a,
                                     idx_b=None if self._same else self._idx_b, dimensions=self._pair_boxes, axes=self._dim)
        return out, None

    def _store(self, sums, _):
        S, r = self._store_gated(sums), self.results
        with np.errstate(divide="ignore", invalid="ignore"):
            r.c1 = np.where(r.count > 0, S[:, 0] / r.count, np.nan)
            r.c2 = np.where(r.count > 0, (3.0 * S[:, 1] / r.count - 1.0) / 2.0, np.nan)
        r.tau_1 = _trapezoid(r.c1, r.times)
        r.tau_2 = _trapezoid(r.c2, r.times)
