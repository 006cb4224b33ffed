"""The shell-resolved reorientation (ta_shell_orient, ShellOrientation) on the CPU backend (Context("cpu"), device="cpu"):
equality with shell_orient_ref's exact integers under both conditions, in the three modes, without a box, in a constant box
and in per-frame boxes (partners wrapped through faces), with the anchor in column 0 and 1, on float64 and float32 slabs;
constructed runs with hand-computed counts; the always-inside case against ta_orient; a degenerate vector; the class's sorting
of rows; every refusal."""
import ctypes
import os
import warnings

import numpy as np
import pytest

import pair_ref
import shell_orient_ref as oref
import shell_ref as ref
from test_pair_lifetime import cpu_context
from transport_analysis_amd import ShellMSD, ShellOrientation, _lib
from transport_analysis_amd._base import UpdatingAtomGroup
from transport_analysis_amd._mini_mda import ArrayUniverse

T = 70  # two 64-frame words


def assert_sums(got, want, what=""):
    for name, g, w in zip(("sums", "count", "runs", "nb"), got, want):
        assert np.array_equal(g, w), (what, name, np.argwhere(np.asarray(g) != np.asarray(w))[:5].tolist())
    assert got[0].dtype == np.float64 and got[0].shape[1] == 2 and got[1].dtype == np.int64 and got[2].dtype == np.int64


# ---- 1. the library call against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", oref.MODES)
@pytest.mark.parametrize("anchor", [0, 1])
def test_against_reference(anchor, mode):
    """walks of 70 frames, 7 reference items and 45 anchors (or one list of 45: idx_b None): no box, the constant box,
    per-frame boxes; gap 0 and 2 with hysteresis; float64 and float32 slabs; both conditions; L = 40 and T - 1"""
    for kind, boxed, gap, L in (("disjoint", False, 0, 40), ("disjoint", True, 2, T - 1), ("disjoint", "frames", 2, 40),
                                ("same", True, 0, 40), ("same", "frames", 2, T - 1)):
        x, a, b, rows, dims, axes, cuts, g, want, runs, nb = oref.case(T, 7, 45, kind, boxed, gap, L, mode, anchor)
        assert 0 < nb.sum() < g.size, "the case must have anchors inside and outside"
        assert want["continuous"][0][1:, 1].any() and (want["continuous"][0][:, 1] < want["continuous"][1]).any()
        for dtype in (np.float64, np.float32):
            c = cpu_context(x, dtype)
            try:
                for condition in oref.CONDITIONS:
                    got = c.shell_orient(condition, L, rows, mode, anchor=anchor, gap=gap, idx_a=a, idx_b=b, dimensions=dims, axes=axes,
                                         **cuts)
                    assert_sums(got, want[condition] + (runs, nb), (kind, boxed, gap, L, dtype.__name__, condition))
            finally:
                c.close()


def test_threads_and_outputs_one_at_a_time():
    x, a, b, rows, dims, axes, cuts, g, want, runs, nb = oref.case(T, 7, 45, "disjoint", True, 1, 40, "bisector")
    full = want["endpoints"] + (runs, nb)
    kw = dict(gap=1, idx_a=a, idx_b=b, dimensions=dims, axes=axes, **cuts)
    c = cpu_context(x)
    try:
        for threads in (1, 3):
            c.set_option("cpu_threads", threads)
            assert_sums(c.shell_orient("endpoints", 40, rows, "bisector", **kw), full)
        for i, key in enumerate(("sums", "count", "runs", "nb")):
            only = c.shell_orient("endpoints", 40, rows, "bisector", **{k: k == key for k in ("sums", "count", "runs", "nb")}, **kw)
            assert [v is not None for v in only] == [j == i for j in range(4)] and np.array_equal(only[i], full[i])
    finally:
        c.close()


# ---- 2. constructed runs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 128])
def test_one_run_of_n_frames(n):
    """a run of exactly n frames from frame 3 on in 200 frames: N(tau) = max(0, n - tau) under both conditions; the vector
    turns by a quarter every 5 frames, so S1(tau) is counted by hand as well"""
    lv = np.zeros((1, 200))
    lv[0, 3:3 + n] = 2
    x, a, b = ref.pattern_positions(lv, n_ref=1)
    phase = (np.arange(200) // 5) % 4
    e = np.array([[1.0, 0, 0], [0, 1.0, 0], [-1.0, 0, 0], [0, -1.0, 0]])[phase]  # (T, 3)
    x = np.concatenate([x, x[:, b] + 0.125 * e[:, None, :]], axis=1)
    rows = np.array([[b[0], x.shape[1] - 1]], dtype=np.int32)
    assert np.array_equal(ref.levels(x, a, b, None, **ref.PATTERN_CUTS), lv)
    L = 140
    hand_n = [max(0, n - tau) for tau in range(L + 1)]
    dots = {0: 1, 1: 0, 2: -1, 3: 0}
    hand_s1 = [sum(dots[(phase[t + tau] - phase[t]) % 4] for t in range(3, 3 + n - tau)) for tau in range(L + 1)]
    hand_s2 = [sum(dots[(phase[t + tau] - phase[t]) % 4] ** 2 for t in range(3, 3 + n - tau)) for tau in range(L + 1)]
    for dtype in (np.float64, np.float32):
        c = cpu_context(x, dtype)
        try:
            for condition in oref.CONDITIONS:
                S, N, runs, nb = c.shell_orient(condition, L, rows, "bond", idx_a=a, idx_b=b, **ref.PATTERN_CUTS)
                assert N.tolist() == hand_n and S[:, 0].tolist() == hand_s1 and S[:, 1].tolist() == hand_s2
                assert runs[n] == 1 and runs.sum() == 1 and nb.sum() == n
        finally:
            c.close()


# ---- 3. always inside: ta_orient's sums -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", oref.MODES)
def test_always_inside_against_orient(mode):
    """a huge r_cut, no box, "continuous", max_lag = T - 1: every term counts, N[tau] = n_b (T - tau), and S1[tau],
    S2[tau] - N[tau] / 3 are (T - tau) times ta_orient's c1, c2 with fft = 0, within the library's 1e-10 of the series' maximum
    (the two routes divide and add in another order: no bit equality is asked for)"""
    rng = np.random.default_rng(11)
    n, nv = 50, 9
    K = oref.ROW_LEN[mode]
    x = np.cumsum(rng.normal(scale=0.1, size=(n, 2 + K * nv, 3)), axis=0) + rng.uniform(0, 3, size=(1, 2 + K * nv, 3))
    rows = (2 + np.arange(K * nv).reshape(K, nv).T).astype(np.int32)  # anchors 2 ... 2 + nv - 1: increasing
    c = cpu_context(x)
    try:
        S, N, runs, nb = c.shell_orient("continuous", n - 1, rows, mode, 1.0e6, idx_a=[0, 1], idx_b=rows[:, 0])
        c1, c2, _, _ = c.orient(0, rows, mode, total=False, collective=False)
    finally:
        c.close()
    norm = (n - np.arange(n)).astype(np.float64)
    assert np.array_equal(N, nv * (n - np.arange(n))) and np.all(nb == nv)
    for got, want in ((S[:, 0], c1 * norm), (S[:, 1] - N / 3.0, c2 * norm)):
        err, bound = np.abs(got - want).max(), 1e-10 * np.abs(want).max()
        print(f"    {mode}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound


# ---- 4. a degenerate vector -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", oref.MODES)
def test_degenerate_vector(mode):
    """one vector's atoms coincide in every frame, another's in every third: zeros in the sums, counted in N; S1[0] is the
    number of non-degenerate terms at lag 0; nothing is NaN"""
    x, a, b, dims, axes, cuts, s, _ = ref.case(T, 3, 5, 3, "disjoint", True, 1)
    box = dims[:, :3]
    g = ref.filtered(s, 1)
    first, second = np.argsort(-g.sum(axis=1), kind="stable")[:2]  # (the two vectors that are inside most often)
    zero = np.zeros((5, T), dtype=bool)
    zero[first] = True
    zero[second, ::3] = True
    x2, rows = oref.with_partners(x, b, mode, 0, box, 3, zero=zero)
    u = oref.unit_vectors(x2, rows, mode, box)
    assert not u[first].any() and g[first].any() and g[second, ::3].any()
    c = cpu_context(x2)
    try:
        for condition in oref.CONDITIONS:
            want = oref.gated_sums(u, g, 40, condition)
            S, N, _, _ = c.shell_orient(condition, 40, rows, mode, gap=1, idx_a=a, idx_b=b, dimensions=dims, axes=axes, **cuts)
            assert np.array_equal(S, want[0]) and np.array_equal(N, want[1]) and np.all(np.isfinite(S))
            assert N[0] == g.sum() and S[0, 0] == (g & ~zero).sum() < N[0]
    finally:
        c.close()


# ---- the class ------------------------------------------------------------------------------------------------------------------
def class_case(mode, anchor, boxed, kind="disjoint", L=30, n_frames=40):
    x, a, b, rows, dims, axes, cuts, g, want, runs, nb = oref.case(n_frames, 6, 30, kind, boxed, 1, L, mode, anchor)
    u = ArrayUniverse(positions=x, dimensions=dims)
    anchors = a if b is None else b
    # the followed group: the anchors and their partners, in an order of its own; vectors are positions within it
    members = np.concatenate([np.unique(rows[:, [j for j in range(rows.shape[1]) if j != anchor]]), anchors[::-1]])
    where = {int(m): i for i, m in enumerate(members)}
    vectors = np.array([[where[int(m)] for m in row] for row in rows])
    return u, u.atoms[a], u.atoms[members], vectors, cuts, want, runs, nb


@pytest.mark.parametrize("stage_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mode,anchor,boxed,kind", [("bond", 0, True, "disjoint"), ("bisector", 1, "frames", "disjoint"),
                                                    ("normal", 0, False, "disjoint"), ("bond", 1, True, "same")])
def test_class_against_reference(mode, anchor, boxed, kind, stage_dtype):
    """every result from the reference's integers; a permuted `vectors` gives equal results (the rows are sorted by anchor)"""
    u, reference, group, vectors, cuts, want, runs, nb = class_case(mode, anchor, boxed, kind)
    kw = dict(mode=mode, anchor=anchor, r_cut=cuts["r_cut"], r_break=cuts["r_break"], intermittency=1, max_lag=30, periodic=bool(boxed),
              device="cpu", stage_dtype=stage_dtype)
    perm = np.random.default_rng(4).permutation(vectors.shape[0])
    for condition in oref.CONDITIONS:
        S, N = want[condition]
        a = ShellOrientation(reference, group, vectors, condition=condition, **kw).run()
        r = a.results
        assert np.array_equal(r.count, N) and np.array_equal(r.run_lengths, runs) and np.array_equal(r.n_inside, nb)
        assert r.mean_inside == float(np.mean(nb)) and r.times.shape == (31,) and r.times[1] == a.times[1] - a.times[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            c1 = np.where(N > 0, S[:, 0] / N, np.nan)
            c2 = np.where(N > 0, (3.0 * S[:, 1] / N - 1.0) / 2.0, np.nan)
            n0 = np.cumsum(nb)[::-1][:31].astype(np.float64)
            assert np.array_equal(r.survival, N / n0, equal_nan=True)
        assert np.array_equal(r.c1, c1, equal_nan=True) and np.array_equal(r.c2, c2, equal_nan=True)
        assert r.c1[0] == 1.0 and r.c2[0] == 1.0
        assert r.tau_1 == float(np.sum(0.5 * (c1[1:] + c1[:-1]) * np.diff(r.times))) or np.isnan(r.tau_1)
        assert r.tau_2 == float(np.sum(0.5 * (c2[1:] + c2[:-1]) * np.diff(r.times))) or np.isnan(r.tau_2)
        p = ShellOrientation(reference, group, vectors[perm], condition=condition, **kw).run().results
        for key in ("count", "c1", "c2", "n_inside", "run_lengths", "survival"):
            assert np.array_equal(getattr(p, key), getattr(r, key), equal_nan=True), key
        if kind == "disjoint":  # the shell is ShellMSD's of the anchors
            m = ShellMSD(reference, group[vectors[:, anchor]], condition=condition, **{k: v for k, v in kw.items() if k not in ("mode", "anchor")})
            assert np.array_equal(m.run().results.count, r.count)


def test_default_max_lag_count_zero_and_never_inside():
    u, reference, group, vectors, cuts, want, runs, nb = class_case("bond", 0, True, L=39)
    r = ShellOrientation(reference, group, vectors, device="cpu", intermittency=1, **cuts).run().results
    assert r.count.shape == (40,) and np.array_equal(r.count, want["continuous"][1])
    zero = r.count == 0
    assert zero.any() and np.all(np.isnan(r.c1[zero])) and np.all(np.isnan(r.c2[zero])) and np.all(np.isfinite(r.c1[~zero]))
    assert np.isnan(r.tau_1) and np.isnan(r.tau_2)
    x, a, b = ref.pattern_positions(np.zeros((3, 9)), n_ref=2)
    x = np.concatenate([x, x[:, b] + np.array([0.0, 0.125, 0.0])], axis=1)
    un = ArrayUniverse(positions=x)
    vec = np.stack([np.arange(3), 3 + np.arange(3)], axis=1)
    with pytest.warns(UserWarning, match="ShellOrientation: no anchor atom is inside the shell in any frame"):
        r = ShellOrientation(un.atoms[a], un.atoms[2:], vec, periodic=False, device="cpu", **ref.PATTERN_CUTS).run().results
    assert not r.count.any() and not r.n_inside.any() and np.all(np.isnan(r.c1)) and np.all(np.isnan(r.c2)) and np.all(np.isnan(r.survival))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        r = ShellOrientation(un.atoms[a], un.atoms[2:], vec, r_cut=1.0e3, periodic=False, device="cpu", devices=None).run().results
    assert np.all(r.count == 3 * np.arange(9, 0, -1)) and np.all(r.c1 == 1.0) and np.all(r.c2 == 1.0) and r.tau_1 == 8.0


def test_docstring_states_the_normalisation():
    doc = " ".join(ShellOrientation.__doc__.split())
    assert "RATIO OF SUMS" in doc and "MDAnalysis averages the per-origin means" in doc
    assert '``condition="endpoints"`` is ``WaterOrientationalRelaxation``\'s selection' in doc


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_class_refusals():
    x, a, b = ref.pattern_positions(np.zeros((3, 9)), n_ref=2)
    x = np.concatenate([x, x[:, b] + 0.125], axis=1)  # atoms 0, 1: reference; 2, 3, 4: anchors; 5, 6, 7: partners
    ua = ArrayUniverse(positions=x, dimensions=[16.0, 16.0, 16.0, 90.0, 90.0, 90.0])
    ref_g, grp = ua.atoms[[0, 1]], ua.atoms[2:]
    vec = np.stack([np.arange(3), 3 + np.arange(3)], axis=1)
    new = lambda *args, **kw: ShellOrientation(*(args or (ref_g, grp, vec)), **{"r_cut": 1.0, **kw})  # noqa: E731
    with pytest.raises(TypeError):
        ShellOrientation(ref_g, grp, vec)  # r_cut is required
    with pytest.raises(TypeError, match="ShellOrientation does not take fft="):
        new(fft=False)
    with pytest.raises(TypeError, match="ShellOrientation does not take compound="):
        new(compound=np.arange(6) // 2)
    with pytest.raises(TypeError, match="ShellOrientation does not take reference_frame="):
        new(reference_frame="barycentric")
    with pytest.raises(TypeError, match="ShellOrientation does not take unwrap="):
        new(unwrap=True)
    with pytest.raises(TypeError, match="by_particle=True is not supported"):
        new(by_particle=True)
    with pytest.raises(TypeError, match="UpdatingAtomGroups are not valid for shell orientation computation"):
        new(UpdatingAtomGroup(), grp, vec)
    with pytest.raises(ValueError, match="ShellOrientation: devices=\\[...\\] with more than one member is not supported"):
        new(devices=[0, 1])
    with pytest.raises(ValueError, match="ShellOrientation: distributed=True is not supported"):
        new(distributed=True)
    with pytest.raises(ValueError, match="ShellOrientation needs dim_type='xyz'"):
        new(dim_type="xy")
    with pytest.raises(ValueError, match="condition must be one of"):
        new(condition="both")
    with pytest.raises(ValueError, match="mode: 'arm', expected one of"):
        new(mode="arm")
    for bad in (-1, 2, 0.5):
        with pytest.raises(ValueError, match="anchor must be a column of vectors, 0 ... 1"):
            new(anchor=bad)
    with pytest.raises(ValueError, match="vectors: shape \\(3, 2\\)"):
        new(mode="normal")
    with pytest.raises(ValueError, match="vectors: entries must be positions within the group, 0 ... 5"):
        new(ref_g, grp, vec + 1)
    with pytest.raises(ValueError, match="vectors: row 1 names an atom twice"):
        new(ref_g, grp, [[0, 3], [1, 1]])
    with pytest.raises(ValueError, match="vectors: two rows share an anchor atom"):
        new(ref_g, grp, [[0, 3], [0, 4]])
    with pytest.raises(ValueError, match="reference and observed overlap but differ"):
        new(ua.atoms[[0, 1, 2]], grp, vec)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="max_lag must be an integer >= 0"):
            new(max_lag=bad)
    with pytest.raises(ValueError, match="max_lag must be at most 2047"):
        new(max_lag=2048)
    with pytest.raises(ValueError, match="max_lag = 9 needs more than the 9 analysed frames"):
        new(max_lag=9, device="cpu").run()
    with pytest.raises(ValueError, match="r_break must be finite and at least r_cut"):
        new(r_break=0.5)
    with pytest.raises(ValueError, match="intermittency must be an integer 0 ... 63"):
        new(intermittency=64)
    u = ArrayUniverse(positions=x)
    with pytest.raises(ValueError, match="needs the periodic box"):
        ShellOrientation(u.atoms[[0, 1]], u.atoms[2:], vec, r_cut=1.0, device="cpu").run()
    # accepted: a non-anchor atom that belongs to the reference group
    r = new(ref_g, ua.atoms[[2, 0]], [[0, 1]], max_lag=8, device="cpu").run().results
    assert r.count.shape == (9,)


# ---- 5, 6. the C-ABI's argument checks ------------------------------------------------------------------------------------------
def test_argument_checks_with_messages():
    L = _lib.lib()
    n_frames, n_atoms = 7, 13
    x = pair_ref.positions(n_frames, n_atoms, 3)
    c = cpu_context(x)
    flat = cpu_context(x[:, :, :2])
    empty = _lib.Context("cpu")
    dims = pair_ref.dimensions(pair_ref.BOX, n_frames)  # (4, 2, 8)
    axes = np.array([0, 1, 2], dtype=np.int32)
    sums, count = np.full((n_frames, 2), -7.0), np.full(n_frames, -7, dtype=np.int64)
    runs, nb = np.full(n_frames + 1, -7, dtype=np.int64), np.full(n_frames, -7.0)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    i64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731
    i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
    bonds = i32([5, 9], [6, 10], [7, 11], [8, 12])
    triples = i32([5, 9, 0], [6, 10, 1], [7, 11, 2], [8, 12, 3])

    def call(h=None, cond=0, lag=6, mode=0, anchor=0, idx=bonds, ia=i64(0, 1, 2), ib=i64(5, 6, 7, 8), dm=dims, ax=axes, r_cut=0.75,
             r_break=1.0, gap=1, o_sums=sums, o_count=count, o_runs=runs, o_nb=nb):
        return L.ta_shell_orient(h or c._h, cond, lag, mode, anchor, p(idx), 0 if ia is None else ia.size, p(ia),
                                 0 if ib is None else ib.size, p(ib), p(dm), p(ax), r_cut, r_break, gap, p(o_sums), p(o_count), p(o_runs),
                                 p(o_nb))

    def fails(code, match, **kw):
        rc = call(**kw)
        assert rc == code, (rc, match, kw)
        msg = L.ta_last_error(kw.get("h") or c._h).decode()
        assert match in msg, (match, msg)
        assert np.all(sums == -7) and np.all(count == -7) and np.all(runs == -7) and np.all(nb == -7), "a refused call wrote into an output"

    try:
        # ta_shell_msd's
        for bad in (-1, 2):
            fails(-1, "shell_orient: condition must be 0 (continuous) or 1 (endpoints)", cond=bad)
        fails(-1, "shell_orient: the sums, count, runs and nb outputs are all NULL", o_sums=None, o_count=None, o_runs=None, o_nb=None)
        fails(-1, "shell_orient: max_lag must be 0 ... n_frames - 1 = 6", lag=-1)
        fails(-1, "shell_orient: max_lag must be 0 ... n_frames - 1 = 6", lag=7)
        fails(-1, "shell_orient: r_cut must be finite and greater than 0", r_cut=np.nan)
        fails(-1, "shell_orient: r_break must be finite and at least r_cut", r_break=0.5)
        fails(-1, "shell_orient: gap must be 0 ... 63", gap=64)
        fails(-1, "shell_orient: dimensions without axes", ax=None)
        fails(-4, "slabs have not been staged", h=empty._h)
        fails(-1, "shell_orient: index list a: entry 13 is outside 0 ... n_atoms - 1", ia=i64(0, 13))
        fails(-1, "shell_orient: index list b must be strictly increasing", ib=i64(5, 7, 6, 8))
        fails(-1, "shell_orient: the index lists overlap (item 2 is in both) but differ", ib=i64(2, 5))
        fails(-1, "shell_orient: r_break = 1.100000 exceeds half the box length 2.000000 of frame 0", r_break=1.1)
        # the vectors'
        for bad in (-1, 3):
            fails(-1, "shell_orient: mode must be TA_ORIENT_BOND (0), TA_ORIENT_BISECTOR (1) or TA_ORIENT_NORMAL (2)", mode=bad)
        for mode, idx, bad, last in ((0, bonds, -1, 1), (0, bonds, 2, 1), (1, triples, 3, 2), (2, triples, 3, 2)):
            fails(-1, f"shell_orient: anchor must be a column of the index rows, 0 ... {last}", mode=mode, idx=idx, anchor=bad)
        fails(-1, "shell_orient: the index table is NULL", idx=None)
        fails(-1, "shell_orient: the position slab must hold three columns per atom (dim = 2)", h=flat._h, ax=i32(0, 1), dm=None)
        fails(-1, "shell_orient: the box needs the three columns x, y, z (axes {0, 1, 2})", ax=i32(0, 2, 1))
        fails(-1, "shell_orient: index 13 of vector 1 is outside 0 ... n_atoms - 1", idx=i32([5, 9], [6, 13], [7, 11], [8, 12]))
        fails(-1, "shell_orient: index -1 of vector 0 is outside 0 ... n_atoms - 1", idx=i32([5, -1], [6, 10], [7, 11], [8, 12]))
        fails(-1, "shell_orient: vector 2 names an atom twice", mode=1, idx=i32([5, 9, 0], [6, 10, 1], [7, 11, 11], [8, 12, 3]))
        # the anchor against the observed items
        fails(-1, "shell_orient: the anchor of vector 1 (atom 10) is not observed item 1 (atom 6)", anchor=1, idx=i32([9, 5], [6, 10], [11, 7], [12, 8]))
        fails(-1, "shell_orient: the anchor of vector 0 (atom 5) is not observed item 0 (atom 0)", ib=None, ia=i64(0, 1, 2, 3))
        with pytest.raises(ValueError, match="index: 3 rows for 4 observed items"):
            c.shell_orient("continuous", 3, bonds[:3], "bond", 0.75, idx_a=[0, 1, 2], idx_b=[5, 6, 7, 8])
        with pytest.raises(ValueError, match="condition: 'both'"):
            c.shell_orient("both", 3, bonds, "bond", 0.75, idx_a=[0, 1, 2], idx_b=[5, 6, 7, 8])
        # accepted: each output alone, lag 0; the anchors as the reference list (idx_b NULL); no box
        assert call(lag=0, o_sums=None, o_runs=None, o_nb=None) == 0 and count[0] >= 0 and np.all(count[1:] == -7) and np.all(sums == -7)
        count[:] = -7
        assert call(ia=i64(5, 6, 7, 8), ib=None, dm=None, ax=None, o_count=None, o_runs=None, o_nb=None) == 0 and np.all(sums != -7)
        assert call(anchor=1, idx=np.ascontiguousarray(bonds[:, ::-1]), mode=0) == 0
    finally:
        c.close()
        flat.close()
        empty.close()


def test_max_lag_above_the_cap():
    """2100 frames: max_lag 2047 is taken, 2048 names the cap"""
    x = np.zeros((2100, 3, 3))
    x[:, 1, 0], x[:, 2, 0] = 0.25, 0.75
    c = cpu_context(x)
    try:
        S, N, runs, nb = c.shell_orient("continuous", 2047, [[1, 2]], "bond", 0.5, idx_a=[0], idx_b=[1])
        assert np.array_equal(N, 2100 - np.arange(2048)) and np.array_equal(S[:, 0], N) and np.array_equal(S[:, 1], N) and runs[2100] == 1
        with pytest.raises(_lib.TAError, match="shell_orient: max_lag must be at most 2047 \\(eight passes of 256 lags\\)") as e:
            c.shell_orient("continuous", 2048, [[1, 2]], "bond", 0.5, idx_a=[0], idx_b=[1])
        assert e.value.code == -1
    finally:
        c.close()


def test_symbols_in_header_and_exports():
    names = {"ta_shell_orient", "ta_shell_orient_staged"}
    assert names <= set(_lib.EXPORTS) and _lib.lib().ta_abi_version() == 6
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ta_hip.h")).read()
    for name in names:
        assert f"int {name}(ta_ctx *ctx, int condition, int64_t max_lag, int mode, int anchor, const int32_t *h_index" in header, name
        assert hasattr(_lib.lib(), name)
    assert "their sums and counts add" in header and "IS counted in N" in header
