"""Shell residence times (ta_shell_residence, ShellResidence) on the CPU backend (Context("cpu"), device="cpu"): equality with
shell_ref at D = 1, 2, 3 without a box, in a constant box and in per-frame boxes; with ONE reference item the bits of
ta_bond_lifetime on the rows (a_0, q); the hand-over from one reference item's shell to another's as ONE residence; the strict
cutoff, the same list, all and none inside, hysteresis and the tolerated absence; every refusal with its text and code; the
class."""
import ctypes
import os
import warnings

import numpy as np
import pytest

import bond_ref
import pair_ref
import shell_ref as ref
from test_pair_lifetime import DIM_TYPES, cpu_context
from transport_analysis_amd import ShellResidence, _lib
from transport_analysis_amd._base import UpdatingAtomGroup
from transport_analysis_amd._mini_mda import ArrayUniverse

T = 70  # two 64-frame words


def assert_sums(got, want, fft=0, what=""):
    ci, runs, nb = got
    assert np.array_equal(runs, want[1]), (what, np.flatnonzero(runs != want[1])[:5])
    assert np.array_equal(nb, want[2]), (what, np.flatnonzero(nb != want[2])[:5])
    if fft:
        err = float(np.max(np.abs(ci - want[0])))
        print(f"    {what}: fft max |ci - exact| = {err:.3e}, bound {1e-10 * max(float(want[0][0]), 1.0):.3e}")
        assert err <= 1e-10 * max(float(want[0][0]), 1.0)
    else:
        assert np.array_equal(ci, want[0]), (what, np.flatnonzero(ci != want[0])[:5])


@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("kind", ["disjoint", "same"])
def test_against_reference(kind, D):
    """walks of 70 frames on the 2^-10 grid, 7 reference and 45 observed items (or one list of 45): no box, the constant box,
    per-frame boxes; gap 0 and 2; float64 and float32 slabs; exact with fft = 0, within 1e-10 of ci[0] with fft = 1"""
    seen = set()
    for boxed in (False, True, "frames"):
        for gap in (0, 2):
            x, a, b, dims, axes, cuts, s, want = ref.case(T, 7, 45, D, kind, boxed, gap)
            seen |= set(np.unique(s).tolist())
            assert 0 < want[2].sum() < s.size, "the case must have items inside and outside"
            for dtype in (np.float64, np.float32):
                c = cpu_context(x, dtype)
                try:
                    for fft in (0, 1):
                        got = c.shell_residence(fft, gap=gap, idx_a=a, idx_b=b, dimensions=dims, axes=axes, **cuts)
                        assert_sums(got, want, fft, (kind, D, boxed, gap, dtype.__name__))
                finally:
                    c.close()
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("boxed", [False, True, "frames"])
def test_one_reference_item_has_the_bits_of_bond_lifetime(boxed):
    """N_a = 1: the OR runs over one item, and ci, runs, nb are bit-equal to ta_bond_lifetime on the rows (a_0, q)"""
    x, a, b, dims, axes, cuts, s, want = ref.case(T, 1, 30, 3, "disjoint", boxed, 1)
    rows = np.stack([np.full(b.size, a[0]), b], axis=1).astype(np.int32)
    c = cpu_context(x)
    try:
        for fft in (0, 1):
            for gap, r_break in ((0, cuts["r_cut"]), (1, cuts["r_break"])):
                got = c.shell_residence(fft, cuts["r_cut"], r_break=r_break, gap=gap, idx_a=a, idx_b=b, dimensions=dims, axes=axes)
                bond = c.bond_lifetime(fft, rows, cuts["r_cut"], r_break=r_break, gap=gap, dimensions=dims, axes=axes)
                assert all(np.array_equal(p, q) for p, q in zip(got, bond)), (fft, gap)
        assert_sums(c.shell_residence(0, gap=1, idx_a=a, idx_b=b, dimensions=dims, axes=axes, **cuts), want)
    finally:
        c.close()


def test_hand_over_is_one_residence():
    """the feature's point: an item passes from the shell of p1 into that of p2 with no frame outside the group's shell.  The
    shell call counts ONE run of the full length; the pair-resolved call on (p1, q), (p2, q) counts two short ones.  Also
    with the item at level 1 of p2 in the hand-over frames: the break radius of ANY reference item holds the residence."""
    n = 100
    lv = np.full((2, n), 2, dtype=np.int8)
    lv[1, 50:53] = 1
    owner = np.zeros((2, n), dtype=np.int64)
    owner[:, 50:] = 1
    x, a, b = ref.pattern_positions(lv, owner, n_ref=2)
    assert np.array_equal(ref.levels(x, a, b, None, **ref.PATTERN_CUTS), lv)
    c = cpu_context(x)
    try:
        for q in range(2):
            ci, runs, nb = c.shell_residence(0, idx_a=a, idx_b=b[q:q + 1], **ref.PATTERN_CUTS)
            assert runs[n] == 1 and runs.sum() == 1 and np.all(nb == 1) and np.array_equal(ci, np.arange(n, 0, -1))
            rows = np.array([[0, b[q]], [1, b[q]]], dtype=np.int32)
            p_ci, p_runs, p_nb = c.bond_lifetime(0, rows, **ref.PATTERN_CUTS)
            assert p_runs.sum() == 2 and p_runs[n] == 0 and p_runs[50] >= 1, "per pair: two short residences"
            assert not np.array_equal(p_runs, runs) and not np.array_equal(p_ci, ci)
        assert_sums(c.shell_residence(0, idx_a=a, idx_b=b, **ref.PATTERN_CUTS), ref.sums(ref.filtered(lv, 0)))
    finally:
        c.close()


def test_strict_cutoffs_and_self():
    """an item exactly on r_cut is outside (level 1 with a larger r_break), exactly on r_break at level 0, one grid step
    inside r_cut at level 2; with the same list an item is never in its own shell"""
    r_cut, r_break = 0.5, 0.75
    x = np.zeros((1, 4, 3))
    x[0, 1, 0], x[0, 2, 1], x[0, 3, 2] = r_cut, r_break, r_cut - 1.0 / 1024
    a, b = np.array([0]), np.array([1, 2, 3])
    assert ref.levels(x, a, b, None, r_cut, r_break)[:, 0].tolist() == [1, 0, 2]
    c = cpu_context(x)
    try:
        for q, level in enumerate([1, 0, 2]):
            assert c.shell_residence(0, r_cut, r_break=r_break, idx_a=a, idx_b=b[q:q + 1])[2][0] == (level == 2)
            assert c.shell_residence(0, r_break, idx_a=a, idx_b=b[q:q + 1])[2][0] == (level >= 1)
        # the same list: item 0 alone is never inside; items 0 and 3 are in each other's shell, 1 and 2 in nobody's
        for lists in (dict(idx_a=[0], idx_b=[0]), dict(idx_a=[0]), dict(idx_a=[1, 2])):
            assert not c.shell_residence(0, r_cut, **lists)[2].any()
        assert c.shell_residence(0, r_cut, idx_a=[0, 3])[2][0] == 2
        assert c.shell_residence(0, r_cut)[2][0] == 2 and c.shell_residence(0, r_cut, idx_a=[0, 1, 2, 3], idx_b=[0, 1, 2, 3])[2][0] == 2
    finally:
        c.close()


def test_all_inside_and_none_inside():
    n, N = 130, 5
    for level, inside in ((2, True), (0, False), (1, False)):
        x, a, b = ref.pattern_positions(np.full((N, n), level), n_ref=3)
        c = cpu_context(x, np.float32)
        try:
            ci, runs, nb = c.shell_residence(0, idx_a=a, idx_b=b, gap=3, **ref.PATTERN_CUTS)
            assert np.all(nb == (N if inside else 0)) and runs.sum() == (N if inside else 0) and runs[n] == (N if inside else 0)
            assert np.array_equal(ci, N * np.arange(n, 0, -1) if inside else np.zeros(n))
        finally:
            c.close()


@pytest.mark.parametrize("gap", [0, 1, 2, 63])
def test_hysteresis_and_intermittency_patterns(gap):
    """bond_ref.constructed_levels at T = 300 (absences of exactly gap and gap + 1 frames inside a word and across word edges,
    the hysteresis carry through whole words, level 1 before the first 2, level 1 only) realised around three reference
    items with the owner changing from frame to frame: all rows at once, and each row alone"""
    lv = bond_ref.constructed_levels(300, gap)
    g = ref.filtered(lv, gap)
    assert np.array_equal(g, bond_ref.filtered(lv, gap))
    owner = (np.arange(lv.shape[0])[:, None] + np.arange(300)[None, :] // 7) % 3
    x, a, b = ref.pattern_positions(lv, owner, n_ref=3)
    assert np.array_equal(ref.levels(x, a, b, None, **ref.PATTERN_CUTS), lv)
    for dtype, threads in ((np.float64, 1), (np.float32, 3)):
        c = cpu_context(x, dtype)
        try:
            c.set_option("cpu_threads", threads)
            assert_sums(c.shell_residence(0, idx_a=a, idx_b=b, gap=gap, **ref.PATTERN_CUTS), ref.sums(g))
            for n in range(lv.shape[0]):
                _, _, nb = c.shell_residence(0, idx_a=a, idx_b=b[n:n + 1], gap=gap, ci=False, runs=False, **ref.PATTERN_CUTS)
                assert np.array_equal(nb.astype(bool), g[n]), (n, np.flatnonzero(nb.astype(bool) != g[n])[:8])
        finally:
            c.close()
    if gap:
        assert g[0, 5:5 + gap].all() and not g[1, 5:5 + gap + 1].any()


def test_intermittency_one_more_than_the_absence():
    """an absence of 5 frames: left open by intermittency 4, closed by 5 and by 6; 63 closes an absence of 63 and not of 64"""
    n = 200
    lv = np.zeros((2, n), dtype=np.int8)
    lv[0, 10:20], lv[0, 25:30] = 2, 2          # absent in frames 20 ... 24
    lv[1, 3], lv[1, 67], lv[1, 132] = 2, 2, 2  # absences of 63 and of 64 frames
    x, a, b = ref.pattern_positions(lv, n_ref=2)
    c = cpu_context(x)
    try:
        for gap, closed in ((0, False), (1, False), (4, False), (5, True), (6, True), (63, True)):
            _, runs, nb = c.shell_residence(0, idx_a=a, idx_b=b[:1], gap=gap, ci=False, **ref.PATTERN_CUTS)
            assert bool(nb[20:25].all()) == closed and bool(nb[20:25].any()) == closed
            assert (runs[20] == 1) == closed and nb.sum() == (20 if closed else 15)
        _, runs, nb = c.shell_residence(0, idx_a=a, idx_b=b[1:], gap=63, ci=False, **ref.PATTERN_CUTS)
        assert nb[3:68].all() and not nb[68:132].any() and runs[65] == 1 and runs[1] == 1
        for gap in (1, 5, 63):
            assert_sums(c.shell_residence(0, idx_a=a, idx_b=b, gap=gap, **ref.PATTERN_CUTS), ref.sums(ref.filtered(lv, gap)))
    finally:
        c.close()


# ---- the C-ABI's argument checks ------------------------------------------------------------------------------------------
def test_argument_checks_with_messages():
    L = _lib.lib()
    n_frames, n_atoms, D = 7, 13, 3
    x = pair_ref.positions(n_frames, n_atoms, D)
    c = cpu_context(x)
    empty = _lib.Context("cpu")
    dims = pair_ref.dimensions(pair_ref.BOX, n_frames)  # (4, 2, 8)
    axes = np.array([0, 1, 2], dtype=np.int32)
    ci, runs, nb = np.full(n_frames, -7.0), np.full(n_frames + 1, -7, dtype=np.int64), np.full(n_frames, -7.0)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    i64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731

    def call(h=None, fft=0, ia=i64(0, 1, 2), ib=i64(5, 6, 7, 8), na=None, nb_=None, dm=dims, ax=axes, r_cut=0.75, r_break=1.0,
             gap=1, o_ci=ci, o_runs=runs, o_nb=nb):
        na = (0 if ia is None else ia.size) if na is None else na
        nb_ = (0 if ib is None else ib.size) if nb_ is None else nb_
        return L.ta_shell_residence(h or c._h, fft, na, p(ia), nb_, p(ib), p(dm), p(ax), r_cut, r_break, gap, p(o_ci), p(o_runs), p(o_nb))

    def fails(code, match, **kw):
        rc = call(**kw)
        assert rc == code, (rc, match, kw)
        msg = L.ta_last_error(kw.get("h") or c._h).decode()
        assert match in msg, (match, msg)
        assert np.all(ci == -7) and np.all(runs == -7) and np.all(nb == -7), "a refused call wrote into an output"

    def boxes(row, frame):
        d = dims.copy()
        d[frame] = row
        return d

    try:
        fails(-1, "fft must be 0 or 1", fft=2)
        fails(-1, "shell_residence: the ci, runs and nb outputs are all NULL", o_ci=None, o_runs=None, o_nb=None)
        fails(-1, "shell_residence: n_a must be >= 1", na=0)
        fails(-1, "shell_residence: n_b must be >= 1", nb_=0)
        for bad in (np.nan, np.inf, 0.0, -0.5):
            fails(-1, "shell_residence: r_cut must be finite and greater than 0", r_cut=bad)
        for bad in (0.5, np.nan, np.inf):
            fails(-1, "shell_residence: r_break must be finite and at least r_cut", r_break=bad)
        for bad in (-1, 64):
            fails(-1, "shell_residence: gap must be 0 ... 63", gap=bad)
        fails(-1, "shell_residence: dimensions without axes", ax=None)
        fails(-4, "slabs have not been staged", h=empty._h)
        fails(-1, "shell_residence: index list a: entry 13 is outside 0 ... n_atoms - 1", ia=i64(0, 13))
        fails(-1, "shell_residence: index list b: entry -1 is outside 0 ... n_atoms - 1", ib=i64(-1, 4))
        fails(-1, "shell_residence: index list a must be strictly increasing", ia=i64(0, 2, 2))
        fails(-1, "shell_residence: index list b must be strictly increasing", ib=i64(6, 5))
        fails(-1, "shell_residence: the index lists overlap (item 2 is in both) but differ: they must be one list or disjoint",
              ib=i64(2, 5))
        fails(-1, "shell_residence: axes: every entry must be 0, 1 or 2", ax=np.array([0, 1, 3], dtype=np.int32))
        fails(-1, "shell_residence: a non-orthogonal box is not supported (the one-step image is not the minimum image there)",
              dm=boxes([4.0, 2.0, 8.0, 90, 60, 90], 2))
        fails(-1, "shell_residence: r_break = 1.100000 exceeds half the box length 2.000000 of frame 0", r_break=1.1)
        fails(-1, "exceeds half the box length 1.500000 of frame 6", dm=boxes([4.0, 1.5, 8.0, 90, 90, 90], 6))
        with pytest.raises(_lib.TAError, match="shell_chunk: 0 \\(automatic\\) or the 64-frame words per pass"):
            c.set_option("shell_chunk", -1)
        # accepted: r_break exactly half the shortest box, gap 63, each output alone, the same list twice, no lists, no box
        assert call(gap=63, o_ci=None, o_nb=None) == 0 and np.all(runs >= 0) and np.all(ci == -7) and np.all(nb == -7)
        runs[:] = -7
        assert call(ib=i64(0, 1, 2), o_ci=None, o_runs=None) == 0 and np.all(nb >= 0)
        nb[:] = -7
        assert call(ia=None, ib=None, dm=None, ax=None, o_runs=None, o_nb=None) == 0 and np.all(ci >= 0)
        ci[:] = -7
        with pytest.raises(ValueError, match="idx_a: shape \\(2, 2\\), expected a 1-d list of item indices"):
            c.shell_residence(0, 1.0, idx_a=np.zeros((2, 2), dtype=np.int64))
        with pytest.raises(ValueError, match="expected \\(7, 6\\)"):
            c.shell_residence(0, 1.0, dimensions=np.zeros((3, 6)))
    finally:
        c.close()
        empty.close()


def test_symbols_in_header_and_exports():
    names = {"ta_shell_residence", "ta_shell_residence_staged"}
    assert names <= set(_lib.EXPORTS) and _lib.lib().ta_abi_version() == 6
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ta_hip.h")).read()
    for name in names:
        assert f"int {name}(ta_ctx *ctx, int fft, int64_t n_a, const int64_t *h_idx_a" in header, name
        assert hasattr(_lib.lib(), name)
    assert '"shell_chunk" n' in header
    assert not hasattr(_lib.lib(), "ta_group_shell_residence")


# ---- the class ----------------------------------------------------------------------------------------------------------------
def universe(x, dims, axes):
    x3 = np.zeros(x.shape[:2] + (3,))
    x3[:, :, list(axes)] = x
    return ArrayUniverse(positions=x3, dimensions=dims)


def class_against_reference(kind, D, boxed, gap, **place):
    """ShellResidence on shell_ref.case(40 frames, 6 reference, 30 observed): every result from the reference's integers"""
    n = 40
    x, a, b, dims, axes, cuts, s, (ci, runs, nb, cc) = ref.case(n, 6, 30, D, kind, boxed, gap)
    u = universe(x, dims, axes)
    kw = dict(r_cut=cuts["r_cut"], r_break=cuts["r_break"], intermittency=gap, periodic=dims is not None, dim_type=DIM_TYPES[D],
              **{"device": "cpu", **place})
    groups = (u.atoms,) if kind == "same" else (u.atoms[a], u.atoms[b])
    want_i, want_s = pair_ref.correlations(ci, nb, cc)
    r = ShellResidence(*groups, fft=False, **kw).run().results
    assert r.n_inside.dtype == np.int64 and np.array_equal(r.n_inside, nb) and r.mean_inside == float(np.mean(nb))
    assert r.run_lengths.dtype == np.int64 and r.run_lengths.shape == (n + 1,) and np.array_equal(r.run_lengths, runs)
    assert np.array_equal(r.intermittent, want_i, equal_nan=True) and np.array_equal(r.survival, want_s, equal_nan=True)
    assert np.array_equal(r.times, np.arange(n) * 1.0)
    if np.isfinite(want_i).all():
        assert r.tau_intermittent == np.sum(0.5 * (want_i[1:] + want_i[:-1]))
        assert r.tau_residence == np.sum(0.5 * (want_s[1:] + want_s[:-1]))
    assert r.mean_run == (np.arange(n + 1) * runs).sum() / runs.sum()
    assert r.survival[0] == 1.0 == r.intermittent[0]
    ok = np.isfinite(want_i)
    assert np.all(r.survival[ok] <= r.intermittent[ok])
    f = ShellResidence(*groups, fft=True, **kw).run().results
    assert np.array_equal(f.n_inside, nb) and np.array_equal(f.run_lengths, runs) and np.array_equal(f.survival, want_s, equal_nan=True)
    n0 = np.cumsum(nb)[::-1].astype(np.float64)
    err = np.nanmax(np.abs(f.intermittent - want_i) * n0)
    assert err <= 1e-10 * ci[0], err
    return r


@pytest.mark.parametrize("D", [1, 2, 3])
def test_class_against_reference(D):
    for kind, boxed, gap in (("disjoint", False, 0), ("disjoint", True, 2), ("same", "frames", 1)):
        class_against_reference(kind, D, boxed, gap)
    class_against_reference("disjoint", D, True, 1, stage_dtype=np.float32)


def test_class_nothing_inside_and_keywords():
    x, a, b = ref.pattern_positions(np.zeros((3, 9)), n_ref=2)
    u = ArrayUniverse(positions=x)
    with pytest.warns(UserWarning, match="no observed atom is inside the shell in any frame"):
        r = ShellResidence(u.atoms[a], u.atoms[b], periodic=False, device="cpu", **ref.PATTERN_CUTS).run().results
    assert not r.n_inside.any() and not r.run_lengths.any() and r.mean_inside == 0.0
    assert np.all(np.isnan(r.survival)) and np.all(np.isnan(r.intermittent)) and np.isnan(r.mean_run)
    assert np.isnan(r.tau_residence) and np.isnan(r.tau_intermittent)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        x2, a2, b2 = ref.pattern_positions(np.full((3, 9), 2), n_ref=2)
        u2 = ArrayUniverse(positions=x2)
        r = ShellResidence(u2.atoms[a2], u2.atoms[b2], r_cut=0.5, periodic=False, device="cpu", devices=None).run().results
    assert np.all(r.n_inside == 3) and np.all(r.survival == 1.0) and r.run_lengths[9] == 3
    ua = ArrayUniverse(positions=x, dimensions=[16.0, 16.0, 16.0, 90.0, 90.0, 90.0])
    with pytest.raises(TypeError):
        ShellResidence(ua.atoms)  # r_cut is required
    with pytest.raises(TypeError, match="ShellResidence does not take compound="):
        ShellResidence(ua.atoms, r_cut=1.0, compound=np.arange(5) // 2)
    with pytest.raises(TypeError, match="ShellResidence does not take reference_frame="):
        ShellResidence(ua.atoms, r_cut=1.0, reference_frame="barycentric")
    with pytest.raises(TypeError, match="ShellResidence does not take unwrap="):
        ShellResidence(ua.atoms, r_cut=1.0, unwrap=True)
    with pytest.raises(TypeError, match="ShellResidence does not take pairs=: every observed atom is followed"):
        ShellResidence(ua.atoms, r_cut=1.0, pairs=[[0, 1]])
    with pytest.raises(TypeError, match="ShellResidence does not take search_stride="):
        ShellResidence(ua.atoms, r_cut=1.0, search_stride=2)
    with pytest.raises(TypeError, match="by_particle=True is not supported"):
        ShellResidence(ua.atoms, r_cut=1.0, by_particle=True)
    with pytest.raises(TypeError, match="UpdatingAtomGroups are not valid for shell residence computation"):
        ShellResidence(ua.atoms, UpdatingAtomGroup(), r_cut=1.0)
    with pytest.raises(ValueError, match="ShellResidence: devices=\\[...\\] with more than one member is not supported"):
        ShellResidence(ua.atoms, r_cut=1.0, devices=[0, 1])
    with pytest.raises(ValueError, match="ShellResidence: distributed=True is not supported"):
        ShellResidence(ua.atoms, r_cut=1.0, distributed=True)
    with pytest.raises(ValueError, match="reference and observed overlap but differ"):
        ShellResidence(ua.atoms[[0, 1, 2]], ua.atoms[[2, 3]], r_cut=1.0)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="r_cut must be finite and > 0"):
            ShellResidence(ua.atoms, r_cut=bad)
    with pytest.raises(ValueError, match="r_break must be finite and at least r_cut"):
        ShellResidence(ua.atoms, r_cut=1.0, r_break=0.5)
    for bad in (-1, 64, 1.5):
        with pytest.raises(ValueError, match="intermittency must be an integer 0 ... 63"):
            ShellResidence(ua.atoms, r_cut=1.0, intermittency=bad)
    with pytest.raises(ValueError, match="invalid dim_type"):
        ShellResidence(ua.atoms, r_cut=1.0, dim_type="yx")
    with pytest.raises(ValueError, match="needs the periodic box"):
        ShellResidence(u.atoms, r_cut=1.0, device="cpu").run()
    with pytest.raises(_lib.TAError, match="shell_residence: r_break = 9.000000 exceeds half the box length"):
        ShellResidence(ua.atoms, r_cut=1.0, r_break=9.0, device="cpu").run()
    assert "ratio of sums" in ShellResidence.__doc__.lower().replace("\n", " ")
