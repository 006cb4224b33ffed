"""Bond lifetimes (ta_bond_lifetime, HydrogenBondLifetime, PairLifetime(r_break=, intermittency=)) on the CPU backend
(Context("cpu"), device="cpu"): equality with bond_ref for pairs and triplets, the identity with ta_pair_lifetime, the
invariants of the two filters, the constructed level patterns of the GPU shape tests, every refusal with its text and code,
and the two classes."""
import ctypes

import numpy as np
import pytest

import bond_ref as ref
import pair_ref
from test_pair_lifetime import DIM_TYPES, cpu_context
from transport_analysis_amd import HydrogenBondLifetime, PairLifetime, _lib
from transport_analysis_amd._mini_mda import ArrayUniverse

T, A = 70, 24  # two 64-frame words
CUTS = dict(r_break=ref.R_BREAK, cos_cut=ref.COS_CUT, cos_break=ref.COS_BREAK)


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
@pytest.mark.parametrize("n_at", [2, 3])
def test_against_reference(n_at, D):
    """walks of 70 frames on the 1/32 grid: no box, the constant box, per-frame boxes; gap 0 and 2; float64 and float32 slabs;
    exact with fft = 0, within 1e-10 of ci[0] with fft = 1.  Every level occurs."""
    seen = set()
    for boxed in (False, True, "frames"):
        for gap in (0, 2):
            x, bonds, dims, axes, s, want = ref.case(T, A, D, n_at, boxed, gap)
            seen |= set(np.unique(s).tolist())
            for dtype in (np.float64, np.float32):
                c = cpu_context(x, dtype)
                try:
                    for fft in (0, 1):
                        got = c.bond_lifetime(fft, bonds, ref.R_CUT, gap=gap, dimensions=dims, axes=axes, **CUTS)
                        assert_sums(got, want, fft, (n_at, D, boxed, gap, dtype.__name__))
                finally:
                    c.close()
    assert seen == {0, 1, 2}


def test_identity_with_pair_lifetime():
    """n_at = 2, r_break = r_cut, gap = 0: the bits of ta_pair_lifetime (the cosines are ignored, whatever they are)"""
    for boxed in (False, True, "frames"):
        x, a, b, dims, axes, pairs, sums = pair_ref.case(40, 60, 3, "explicit", boxed, 1)
        c = cpu_context(x)
        try:
            for fft in (0, 1):
                want = c.pair_lifetime(fft, pair_ref.R_CUT, pairs, dimensions=dims, axes=axes)
                got = c.bond_lifetime(fft, pairs, pair_ref.R_CUT, cos_cut=7.0, cos_break=np.nan, dimensions=dims, axes=axes)
                assert all(np.array_equal(p, q) for p, q in zip(got, want))
        finally:
            c.close()


def test_invariants():
    x, bonds, dims, axes, s, _ = ref.case(T, A, 3, 3, True, 0)
    c = cpu_context(x)
    try:
        before = None
        for gap in (0, 1, 2, 5, 63):
            ci, runs, nb = c.bond_lifetime(0, bonds, ref.R_CUT, gap=gap, dimensions=dims, axes=axes, **CUTS)
            assert (np.arange(T + 1) * runs).sum() == nb.sum()
            if before is not None:
                assert np.all(nb >= before), "nb must not decrease with gap"
            before = nb
        # after gap = n no interior absence of <= n frames is left; hysteresis never bonds a series without a level 2
        for n in range(bonds.shape[0]):
            for gap in (1, 3):
                _, _, g = c.bond_lifetime(0, bonds[n:n + 1], ref.R_CUT, gap=gap, dimensions=dims, axes=axes, ci=False, runs=False, **CUTS)
                on = np.flatnonzero(g)
                assert on.size < 2 or np.all((np.diff(on) == 1) | (np.diff(on) > gap + 1))
                if not (s[n] == 2).any():
                    assert not g.any()
        assert any(not (row == 2).any() and (row == 1).any() for row in s), "no series with level 1 only: choose another seed"
    finally:
        c.close()


def test_boundaries():
    """triplets exactly on cos_cut are bonded (the inclusive >=), pairs exactly on r_cut and r_break are not (the strict <)"""
    x, bonds = ref.boundary_triplets()
    s = ref.levels(x, bonds, None, ref.R_CUT, ref.R_BREAK, 0.25, 0.0625)
    assert s[:, 0].tolist() == [2, 0, 2, 1]
    c = cpu_context(x)
    try:
        for n, level in enumerate(s[:, 0]):
            _, _, nb = c.bond_lifetime(0, bonds[n:n + 1], ref.R_CUT, ci=False, runs=False, **CUTS)
            assert nb[0] == (level == 2), (n, level)
            # with the form criterion at the break values a level 1 is a bond
            _, _, nb = c.bond_lifetime(0, bonds[n:n + 1], ref.R_BREAK, cos_cut=ref.COS_BREAK, ci=False, runs=False)
            assert nb[0] == (level >= 1), (n, level)
    finally:
        c.close()
    x, bonds = ref.boundary_pairs()
    assert ref.levels(x, bonds, None, ref.R_CUT, ref.R_BREAK)[:, 0].tolist() == [1, 0, 2]
    c = cpu_context(x)
    try:
        assert c.bond_lifetime(0, bonds, ref.R_CUT, r_break=ref.R_BREAK)[2].tolist() == [1.0]
        assert c.bond_lifetime(0, bonds, ref.R_BREAK)[2].tolist() == [2.0]
    finally:
        c.close()


@pytest.mark.parametrize("gap", [0, 1, 2, 63])
def test_constructed_patterns(gap):
    """bond_ref.constructed_levels at T = 300 (word edges 63|64, 127|128, ...) through pattern_positions: all rows at once,
    and each row alone (the per-frame series itself)"""
    lv = ref.constructed_levels(300, gap)
    g = ref.filtered(lv, gap)
    x, bonds = ref.pattern_positions(lv)
    for dtype, threads in ((np.float64, 1), (np.float32, 3)):
        c = cpu_context(x, dtype)
        try:
            c.set_option("cpu_threads", threads)
            assert_sums(c.bond_lifetime(0, bonds, gap=gap, **ref.PATTERN_CUTS), ref.sums(g))
            for n in range(lv.shape[0]):
                _, _, nb = c.bond_lifetime(0, bonds[n:n + 1], gap=gap, ci=False, runs=False, **ref.PATTERN_CUTS)
                assert np.array_equal(nb.astype(bool), g[n]), (n, np.flatnonzero(nb.astype(bool) != g[n])[:8])
        finally:
            c.close()
    # what the construction is for: absences of exactly gap frames are filled, of gap + 1 are not
    if gap:
        assert g[0, 5:5 + gap].all() and not g[1, 5:5 + gap + 1].any()
    # the carry passes through three whole words; level 1 before the first 2 and level 1 only are not bonded; a 0 breaks
    base = 6 + 2
    assert g[base + 1, 3:4 + 3 * 64 + 11].all() and not g[base + 2, :10].any() and g[base + 2, 10:21].all()
    assert g[base + 3, 2:15].all() and not g[base + 3, 15:].any() and not g[base + 4].any() and g[base + 5, 63:65].all()


# ---- the C-ABI's argument checks ------------------------------------------------------------------------------------------
def test_argument_checks_with_messages():
    L = _lib.lib()
    n_frames, n_atoms, D = 7, 13, 3
    x = pair_ref.positions(n_frames, n_atoms, D)
    c = cpu_context(x)
    empty = _lib.Context("cpu")
    dims = pair_ref.dimensions(pair_ref.BOX, n_frames)  # (4, 2, 8)
    axes = np.array([0, 1, 2], dtype=np.int32)
    tri = np.array([[0, 1, 2], [3, 4, 12]], dtype=np.int32)
    ci, runs, nb = np.full(n_frames, -7.0), np.full(n_frames + 1, -7, dtype=np.int64), np.full(n_frames, -7.0)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731

    def life(h=None, fft=0, n=2, n_at=3, at=tri, dm=dims, ax=axes, r_cut=0.75, r_break=1.0, cc=-0.5, cb=-0.25, gap=1, o_ci=ci,
             o_runs=runs, o_nb=nb):
        return L.ta_bond_lifetime(h or c._h, fft, n, n_at, p(at), p(dm), p(ax), r_cut, r_break, cc, cb, gap, p(o_ci), p(o_runs), p(o_nb))

    def fails(code, match, **kw):
        rc = life(**kw)
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
        fails(-1, "bond_lifetime: the ci, runs and nb outputs are all NULL", o_ci=None, o_runs=None, o_nb=None)
        for bad in (1, 4, 0):
            fails(-1, "bond_lifetime: n_at must be 2 (pairs) or 3 (donor, hydrogen, acceptor)", n_at=bad)
        for bad in (np.nan, np.inf, 0.0, -0.5):
            fails(-1, "bond_lifetime: r_cut must be finite and greater than 0", r_cut=bad)
        for bad in (0.5, np.nan, np.inf):
            fails(-1, "bond_lifetime: r_break must be finite and at least r_cut", r_break=bad)
        for bad in (0.25, -1.5, np.nan, -np.inf):
            fails(-1, "bond_lifetime: cos_cut and cos_break must lie in [-1, 0]", cc=bad, cb=0.0 if bad == 0.25 else -0.25)
            fails(-1, "bond_lifetime: cos_cut and cos_break must lie in [-1, 0]", cc=-1.0, cb=bad)
        fails(-1, "bond_lifetime: cos_break must be at least cos_cut", cc=-0.25, cb=-0.5)
        for bad in (-1, 64):
            fails(-1, "bond_lifetime: gap must be 0 ... 63", gap=bad)
        fails(-1, "bond_lifetime: dimensions without axes", ax=None)
        fails(-4, "slabs have not been staged", h=empty._h)
        fails(-1, "bond_lifetime: n_bonds must be 1 ... 2^30 - 1", n=0)
        fails(-1, "bond_lifetime: n_bonds must be 1 ... 2^30 - 1", n=2 ** 30)
        fails(-1, "bond_lifetime: the atoms list is NULL", at=None)
        fails(-1, "bond_lifetime: bond 1 names item 13 outside 0 ... n_atoms - 1", at=i32(0, 1, 2, 3, 13, 4))
        fails(-1, "bond_lifetime: bond 0 names item -1 outside 0 ... n_atoms - 1", at=i32(0, 1, -1, 3, 4, 5))
        fails(-1, "bond_lifetime: bond 1 names item 3 twice", at=i32(0, 1, 2, 3, 4, 3))
        fails(-1, "bond_lifetime: bond 0 names item 5 twice", n_at=2, at=i32(5, 5, 1, 2))
        fails(-1, "bond_lifetime: a non-orthogonal box is not supported", dm=boxes([4.0, 2.0, 8.0, 90, 60, 90], 2))
        fails(-1, "bond_lifetime: r_break = 1.100000 exceeds half the box length 2.000000 of frame 0", r_break=1.1)
        fails(-1, "exceeds half the box length 1.500000 of frame 6", dm=boxes([4.0, 1.5, 8.0, 90, 90, 90], 6))
        # accepted: r_break exactly half the shortest box, gap 63, cosines on both ends, each output alone; pairs' cosines ignored
        assert life(gap=63, cc=-1.0, cb=0.0, o_ci=None, o_nb=None) == 0 and np.all(runs >= 0) and np.all(ci == -7)
        runs[:] = -7
        assert life(n_at=2, at=i32(0, 1, 2, 3), cc=5.0, cb=np.nan, o_ci=None, o_runs=None) == 0 and np.all(nb >= 0)
        nb[:] = -7
        with pytest.raises(ValueError, match="expected an integer \\(n_bonds, 2\\) or \\(n_bonds, 3\\) array"):
            c.bond_lifetime(0, np.zeros((3, 4), dtype=np.int32), 1.0)
        assert {"ta_bond_lifetime", "ta_bond_lifetime_staged"} <= set(_lib.EXPORTS) and L.ta_abi_version() == 6
    finally:
        c.close()
        empty.close()


# ---- the classes --------------------------------------------------------------------------------------------------------------
def water(n_mol=24, n_frames=40, seed=3, box=8.0):
    """a water-like system on no grid: oxygens on a jittered lattice of spacing 2.7 in a box of 8 (three per axis, 24 of the 27
    sites), two hydrogens 1.0 from each at a wide angle, everything jittering from frame to frame and the molecules turning
    slowly.  Atoms in molecule order O, H, H.  Returns (universe, positions, oxygens, hydrogens, donor-hydrogen pairs)"""
    rng = np.random.default_rng(seed)
    sites = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:n_mol] * 2.7
    x = np.zeros((n_frames, 3 * n_mol, 3))
    axis = rng.normal(size=(n_mol, 3))
    other = rng.normal(size=(n_mol, 3))
    for t in range(n_frames):
        axis += 0.15 * rng.normal(size=axis.shape)
        other += 0.15 * rng.normal(size=other.shape)
        e1 = axis / np.linalg.norm(axis, axis=1, keepdims=True)
        e2 = other - (other * e1).sum(axis=1, keepdims=True) * e1
        e2 /= np.linalg.norm(e2, axis=1, keepdims=True)
        o = sites + 0.25 * rng.normal(size=sites.shape)
        x[t, 0::3] = o
        x[t, 1::3] = o + 1.0 * (np.cos(0.9) * e1 + np.sin(0.9) * e2)
        x[t, 2::3] = o + 1.0 * (np.cos(0.9) * e1 - np.sin(0.9) * e2)
    u = ArrayUniverse(positions=x, dimensions=[box, box, box, 90.0, 90.0, 90.0])
    ox, hy = np.arange(0, 3 * n_mol, 3), np.setdiff1d(np.arange(3 * n_mol), np.arange(0, 3 * n_mol, 3))
    dh = np.stack([np.repeat(ox, 2), hy], axis=1)
    return u, x, ox, hy, dh


def hydrogen_bond_lifetime_on_water(**place):
    u, x, ox, hy, dh = water()
    n_frames = x.shape[0]
    kw = dict(d_a_cutoff=3.2, d_h_a_angle_cutoff=150.0, d_a_break=3.6, angle_break=130.0, intermittency=1, fft=False, **place)
    hb = HydrogenBondLifetime(u.atoms[ox], u.atoms[hy], u.atoms[ox], donor_hydrogen_pairs=dh, **kw).run()
    r = hb.results
    # both directions of every found pair, each with the donor's two hydrogens
    assert r.bonds.shape[1] == 3 and r.bonds.shape[0] % 4 == 0 and r.bonds.shape[0] > 0
    rows = set(map(tuple, r.bonds))
    assert all((a, h2, d) in rows for d, h, a in r.bonds for h2 in (a + 1, a + 2))
    assert all(h in (d + 1, d + 2) for d, h, a in r.bonds)
    # the reference with the class's own float64 squared cosines; no triplet-frame within 1e-9 uu vv of a boundary
    box = np.full((n_frames, 3), 8.0)
    s = ref.levels(x, r.bonds, box, 3.2, 3.6, hb.cos_cut * hb.cos_cut, hb.cos_break * hb.cos_break, margin=1e-9)
    assert set(np.unique(s).tolist()) == {0, 1, 2}, "the seed must give every level"
    h = ref.hysteresis(s)
    g = ref.close_gaps(h, 1)
    assert (h != (s == 2)).any() and (g != h).any(), "the seed must make both filters matter"
    ci, runs, nb, cc = ref.sums(g)
    want_i, want_c = pair_ref.correlations(ci, nb, cc)
    assert np.array_equal(r.n_bonded, nb) and np.array_equal(r.run_lengths, runs)
    assert np.array_equal(r.intermittent, want_i, equal_nan=True) and np.array_equal(r.continuous, want_c, equal_nan=True)
    assert r.coordination == np.mean(nb / float(ox.size))
    # the donor-hydrogen search on frame 0 gives the explicit list's triplets
    found = HydrogenBondLifetime(u.atoms[ox], u.atoms[hy], u.atoms[ox], d_h_cutoff=1.05, **kw).run().results
    assert np.array_equal(found.bonds, r.bonds) and np.array_equal(found.n_bonded, nb) and np.array_equal(found.run_lengths, runs)
    # donors and acceptors as two disjoint groups: one direction
    d_, a_ = ox[::2], ox[1::2]
    one = HydrogenBondLifetime(u.atoms[d_], u.atoms[hy], u.atoms[a_], **kw).run().results
    assert set(one.bonds[:, 0]) <= set(d_) and set(one.bonds[:, 2]) <= set(a_)
    s1 = ref.levels(x, one.bonds, box, 3.2, 3.6, hb.cos_cut * hb.cos_cut, hb.cos_break * hb.cos_break, margin=1e-9)
    assert np.array_equal(one.n_bonded, ref.filtered(s1, 1).sum(axis=0))


def test_hydrogen_bond_lifetime_on_water():
    hydrogen_bond_lifetime_on_water(device="cpu")


def test_hydrogen_bond_lifetime_refusals():
    u, x, ox, hy, dh = water(n_mol=4, n_frames=3)
    D, H = u.atoms[ox], u.atoms[hy]
    with pytest.raises(ValueError, match="HydrogenBondLifetime: devices=\\[...\\] with more than one member is not supported"):
        HydrogenBondLifetime(D, H, D, devices=[0, 1])
    with pytest.raises(ValueError, match="HydrogenBondLifetime: distributed=True is not supported"):
        HydrogenBondLifetime(D, H, D, distributed=True)
    with pytest.raises(TypeError, match="HydrogenBondLifetime does not take compound="):
        HydrogenBondLifetime(D, H, D, compound=np.arange(4))
    with pytest.raises(TypeError, match="HydrogenBondLifetime does not take unwrap=: the minimum image makes unwrapping unnecessary"):
        HydrogenBondLifetime(D, H, D, unwrap=True)
    with pytest.raises(ValueError, match="donors and acceptors overlap but differ"):
        HydrogenBondLifetime(u.atoms[ox[:3]], H, u.atoms[ox[2:]])
    with pytest.raises(ValueError, match="hydrogens must be disjoint from donors and acceptors"):
        HydrogenBondLifetime(D, u.atoms[[0, 1]], D)
    with pytest.raises(ValueError, match="d_h_a_angle_cutoff must lie in 90 ... 180 degrees"):
        HydrogenBondLifetime(D, H, D, d_h_a_angle_cutoff=60.0)
    with pytest.raises(ValueError, match="angle_break must be at most d_h_a_angle_cutoff"):
        HydrogenBondLifetime(D, H, D, angle_break=170.0)
    with pytest.raises(ValueError, match="d_a_break must be finite and at least d_a_cutoff"):
        HydrogenBondLifetime(D, H, D, d_a_break=2.0)
    with pytest.raises(ValueError, match="intermittency must be an integer 0 ... 63"):
        HydrogenBondLifetime(D, H, D, intermittency=64)
    with pytest.raises(ValueError, match="donor_hydrogen_pairs: every row must name an atom of donors and an atom of hydrogens"):
        HydrogenBondLifetime(D, H, D, donor_hydrogen_pairs=[[1, 0]])
    with pytest.raises(ValueError, match="r_break must be finite and at least r_cut"):
        PairLifetime(u.atoms, r_cut=2.0, r_break=1.0)
    with pytest.raises(ValueError, match="intermittency must be an integer 0 ... 63"):
        PairLifetime(u.atoms, r_cut=2.0, intermittency=-1)


def pair_lifetime_with_filters(kind, **place):
    """PairLifetime(r_break=, intermittency=) against the reference on pair_ref's walks (searched and explicit lists); with the
    defaults the results are those of the unfiltered call, bit for bit"""
    case = pair_ref.case(40, 60, 3, kind, True, 1)
    x, a, b, dims, axes, pairs, sums = case
    u = ArrayUniverse(positions=x, dimensions=dims)
    common = dict(r_cut=0.75, fft=False, dim_type=DIM_TYPES[3], **place, **({} if kind == "same" else dict(pairs=pairs)))
    r = PairLifetime(u.atoms, r_break=1.0, intermittency=2, **common).run().results
    s = ref.levels(x, r.pairs, dims[:, :3], 0.75, 1.0)
    g = ref.filtered(s, 2)
    ci, runs, nb, cc = ref.sums(g)
    assert (g != (s == 2)).any()
    assert np.array_equal(r.n_bonded, nb) and np.array_equal(r.run_lengths, runs)
    want_i, want_c = pair_ref.correlations(ci, nb, cc)
    assert np.array_equal(r.intermittent, want_i, equal_nan=True) and np.array_equal(r.continuous, want_c, equal_nan=True)
    plain = PairLifetime(u.atoms, **common).run().results
    again = PairLifetime(u.atoms, r_break=None, intermittency=0, **common).run().results
    want = ref.sums(ref.levels(x, plain.pairs, dims[:, :3], 0.75, 0.75) == 2)
    assert np.array_equal(plain.n_bonded, want[2]) and np.array_equal(plain.run_lengths, want[1])
    for key in ("pairs", "n_bonded", "run_lengths", "intermittent", "continuous"):
        assert np.array_equal(getattr(plain, key), getattr(again, key), equal_nan=True)


@pytest.mark.parametrize("kind", ["same", "explicit"])
def test_pair_lifetime_with_filters(kind):
    pair_lifetime_with_filters(kind, device="cpu")
