"""Pair lifetimes (ta_pair_find, ta_pair_find_read, ta_pair_lifetime, PairLifetime) on the CPU backend (Context("cpu"),
device="cpu"): the reference of pair_ref (found lists, bonded counts, run lengths and the fft=False correlations EQUAL), the
invariants, every refusal of the class and every argument check of the three entry points with its text.  (The one return
that needs a slab of 2^31 columns is reached in test_pair_lifetime_shapes.py on a device-only slab.)"""
import ctypes
import itertools
import warnings

import numpy as np
import pytest

import pair_ref as ref
from transport_analysis_amd import PairLifetime, _lib
from transport_analysis_amd._base import UpdatingAtomGroup
from transport_analysis_amd._mini_mda import ArrayUniverse

T, A = 40, 60
DIM_TYPES = {1: "y", 2: "xz", 3: "xyz"}  # pair_ref.AXES by D


def cpu_context(x, dtype=np.float64):
    n_frames, n_atoms, D = x.shape
    c = _lib.Context("cpu")
    (view,) = c.stage_alloc(n_frames, n_atoms, D, dtype=dtype)
    view[:] = x
    c.stage_commit(0, n_frames)
    return c


def universe(case):
    """the case's D staged columns as the columns `axes` of 3-d positions, with its boxes"""
    x, a, b, dims, axes, pairs, sums = case
    x3 = np.zeros(x.shape[:2] + (3,))
    x3[:, :, list(axes)] = x
    return ArrayUniverse(positions=x3, dimensions=dims)


def run_class(case, kind, stride, fft, **kw):
    """PairLifetime on the case; kw: the class's other keywords, the placement among them (default device="cpu")"""
    x, a, b, dims, axes, pairs, sums = case
    u = universe(case)
    D = x.shape[2]
    common = dict(r_cut=ref.R_CUT, periodic=dims is not None, fft=fft, dim_type=DIM_TYPES[D], **{"device": "cpu", **kw})
    if kind == "same":
        return PairLifetime(u.atoms, search_stride=stride, **common).run()
    if kind == "disjoint":
        return PairLifetime(u.atoms[a], u.atoms[b], search_stride=stride, **common).run()
    return PairLifetime(u.atoms, pairs=pairs, **common).run()


def class_against_reference(kind, D, **place):
    """T = 40, A = 60: no box, the constant box and per-frame boxes, search strides 1 and 3; exact with fft=False, the
    project's 1e-10 of the scale (ci[0]) with fft=True"""
    for boxed, stride in itertools.product((False, True, "frames"), (1, 3)):
        case = ref.case(T, A, D, kind, boxed, stride)
        x, a, b, dims, axes, pairs, sums = case
        what = (kind, D, boxed, stride)
        if sums is None or not sums[2].any():  # (no pair ever bonded: D = 3 walks without a box spread over 50 length units)
            with pytest.warns(UserWarning, match="no pair is bonded"):
                r = run_class(case, kind, stride, False, **place).results
            assert np.array_equal(r.pairs, pairs) and np.all(np.isnan(r.intermittent)) and np.all(np.isnan(r.continuous))
            assert not r.n_bonded.any() and not r.run_lengths.any() and np.isnan(r.mean_run)
            continue
        ci, runs, nb, cc = sums
        want_i, want_c = ref.correlations(ci, nb, cc)
        r = run_class(case, kind, stride, False, **place).results
        assert np.array_equal(r.pairs, pairs), what
        assert r.n_bonded.dtype == np.int64 and np.array_equal(r.n_bonded, nb), what
        assert r.run_lengths.dtype == np.int64 and r.run_lengths.shape == (T + 1,) and np.array_equal(r.run_lengths, runs), what
        assert np.array_equal(r.intermittent, want_i, equal_nan=True), what
        assert np.array_equal(r.continuous, want_c, equal_nan=True), what
        assert np.array_equal(r.times, np.arange(T) * 1.0)
        n_a = A if kind != "disjoint" else a.size
        assert r.coordination == np.mean(nb / float(n_a))
        ok = np.isfinite(want_i)
        if ok.all():
            assert r.tau_intermittent == np.sum(0.5 * (want_i[1:] + want_i[:-1]))
            assert r.tau_continuous == np.sum(0.5 * (want_c[1:] + want_c[:-1]))
        assert r.mean_run == (np.arange(T + 1) * runs).sum() / runs.sum()
        # the invariants
        assert r.intermittent[0] == 1.0 == r.continuous[0]
        assert np.all(r.continuous[ok] <= r.intermittent[ok])
        assert (np.arange(T + 1) * r.run_lengths).sum() == r.n_bonded.sum()
        # fft=True: the same integers for runs and counts, the lag sums within 1e-10 of ci[0]
        f = run_class(case, kind, stride, True, **place).results
        assert np.array_equal(f.pairs, pairs) and np.array_equal(f.n_bonded, nb) and np.array_equal(f.run_lengths, runs)
        n0 = np.cumsum(nb)[::-1].astype(np.float64)
        err = float(np.max(np.abs(f.intermittent[ok] * n0[ok] - ci[ok])))
        print(f"    {what}: fft max |ci - exact| = {err:.3e}, bound {1e-10 * ci[0]:.3e}")
        assert err <= 1e-10 * ci[0]
        assert np.array_equal(f.continuous, want_c, equal_nan=True)


@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("kind", ["same", "disjoint", "explicit"])
def test_class_against_reference(kind, D):
    class_against_reference(kind, D, device="cpu")


@pytest.mark.parametrize("D", [1, 2, 3])
def test_found_pairs_are_exactly_the_pairs_bonded_in_a_searched_frame(D):
    for boxed, stride in itertools.product((False, True, "frames"), (1, 3)):
        x, a, b, dims, axes, pairs, _ = ref.case(T, A, D, "same", boxed, stride)
        box = None if dims is None else dims[:, list(axes)]
        every = ref.all_pairs(np.arange(A), None)
        h = ref.indicator(x, every, box, ref.R_CUT)[:, ::stride].any(axis=1)
        listed = set(map(tuple, pairs))
        assert listed == set(map(tuple, every[h])) and not listed & set(map(tuple, every[~h]))
        c = cpu_context(x)
        try:
            got = c.pair_find(ref.R_CUT, search_stride=stride, dimensions=dims, axes=axes)
            assert got.dtype == np.int32 and np.array_equal(got, pairs)
            # the same list twice is the same list; float32 staging of these values is exact
            assert np.array_equal(c.pair_find(ref.R_CUT, search_stride=stride, idx_a=np.arange(A), idx_b=np.arange(A), dimensions=dims,
                                              axes=axes), pairs)
        finally:
            c.close()
        c = cpu_context(x, np.float32)
        try:
            assert np.array_equal(c.pair_find(ref.R_CUT, search_stride=stride, dimensions=dims, axes=axes), pairs)
        finally:
            c.close()


def test_pairs_exactly_on_the_cutoff_are_not_bonded():
    """the strict <: partners at exactly r_cut = 0.5 (and, across the boundary of a box of 8, at 7.5) are never bonded; at
    0.5 - 2^-10 they are"""
    x = np.zeros((3, 6, 3))
    x[:, 1, 0] = 0.5
    x[:, 2, 1], x[:, 3, 1] = 4.0, 4.0 + 0.5 - 2.0 ** -10
    x[:, 4, 2], x[:, 5, 2] = 0.25, 7.75
    x[:, 4:, 0] = 2.0
    pairs = np.array([[0, 1], [2, 3], [4, 5]])
    c = cpu_context(x)
    try:
        dims = ref.dimensions((8.0, 8.0, 8.0), 3)
        ci, runs, nb = c.pair_lifetime(0, 0.5, pairs, dimensions=dims)
        assert nb.tolist() == [1.0, 1.0, 1.0] and runs.tolist() == [0, 0, 0, 1] and ci.tolist() == [3.0, 2.0, 1.0]
        assert c.pair_find(0.5, dimensions=dims).tolist() == [[2, 3]]
        x2 = x.copy()
        x2[:, 5, 2] = 7.75 + 2.0 ** -10  # (the image distance falls below the cutoff)
    finally:
        c.close()
    c = cpu_context(x2)
    try:
        assert c.pair_find(0.5, dimensions=dims).tolist() == [[2, 3], [4, 5]]
        assert c.pair_find(0.5).tolist() == [[2, 3]]  # (without the box 4 and 5 are 7.5 apart)
    finally:
        c.close()


def test_constructed_patterns_and_runs_across_word_edges():
    """pair_ref.pattern_positions realises given bits: always, never, alternating, single runs over [63, 65], [127, 128] and
    [0, T - 1], at T = 130 (three 64-frame words); the run lengths are those of the construction"""
    n = 130
    names = ("always", "never", "alternating", (63, 65), (127, 128), (0, n - 1), (64, 127), (5, 63))
    bits = np.stack([ref.pattern(k, n) for k in names])
    x, pairs = ref.pattern_positions(bits)
    ci, runs, nb, cc = ref.sums(bits)
    want = np.zeros(n + 1, dtype=np.int64)
    for length, count in ((n, 2), (1, 65), (3, 1), (2, 1), (64, 1), (59, 1)):
        want[length] += count
    assert np.array_equal(runs, want)
    for dtype, threads in ((np.float64, 1), (np.float32, 3)):
        c = cpu_context(x, dtype)
        try:
            c.set_option("cpu_threads", threads)
            c.set_option("pair_chunk", 3)  # (accepted; the CPU backend has no block to chunk)
            got = c.pair_lifetime(0, 0.5, pairs)
            assert np.array_equal(got[0], ci) and np.array_equal(got[1], runs) and np.array_equal(got[2], nb)
            only = c.pair_lifetime(1, 0.5, pairs, ci=False, nb=False)
            assert only[0] is None and only[2] is None and np.array_equal(only[1], runs)
            assert np.array_equal(c.pair_find(0.5), pairs[np.array([k != "never" for k in names])])
        finally:
            c.close()


# ---- the class's refusals -------------------------------------------------------------------------------------------------
def gas(n_frames=3, N=10, box=8.0, seed=0):
    return np.random.default_rng(seed).uniform(0, box, size=(n_frames, N, 3)), [box, box, box, 90.0, 90.0, 90.0]


def test_class_refusals():
    x, dims = gas()
    u = ArrayUniverse(positions=x, dimensions=dims)
    with pytest.raises(ValueError, match="the pairs cross the shards"):
        PairLifetime(u.atoms, r_cut=2.0, devices=[0, 1])
    with pytest.raises(ValueError, match="the pairs cross the blocks"):
        PairLifetime(u.atoms, r_cut=2.0, distributed=True)
    with pytest.raises(TypeError, match="PairLifetime does not take compound="):
        PairLifetime(u.atoms, r_cut=2.0, compound=np.arange(10) // 2)
    with pytest.raises(TypeError, match="PairLifetime does not take reference_frame="):
        PairLifetime(u.atoms, r_cut=2.0, reference_frame="barycentric")
    with pytest.raises(TypeError, match="PairLifetime does not take unwrap=: the minimum image makes unwrapping unnecessary"):
        PairLifetime(u.atoms, r_cut=2.0, unwrap=True)
    with pytest.raises(TypeError, match="by_particle=True is not supported"):
        PairLifetime(u.atoms, r_cut=2.0, by_particle=True)
    with pytest.raises(TypeError, match="UpdatingAtomGroups are not valid for pair lifetime computation"):
        PairLifetime(UpdatingAtomGroup(), r_cut=2.0)
    with pytest.raises(TypeError, match="UpdatingAtomGroups are not valid"):
        PairLifetime(u.atoms, UpdatingAtomGroup(), r_cut=2.0)
    with pytest.raises(TypeError):
        PairLifetime(u.atoms)  # r_cut is required
    with pytest.raises(ValueError, match="more than once"):
        PairLifetime(u.atoms[[0, 1, 1]], r_cut=2.0)
    with pytest.raises(ValueError, match="overlap but differ"):
        PairLifetime(u.atoms[[0, 1, 2]], u.atoms[[2, 3]], r_cut=2.0)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="r_cut must be finite and > 0"):
            PairLifetime(u.atoms, r_cut=bad)
    with pytest.raises(ValueError, match="search_stride must be >= 1"):
        PairLifetime(u.atoms, r_cut=2.0, search_stride=0)
    with pytest.raises(ValueError, match="pairs: a non-empty integer \\(P, 2\\) array"):
        PairLifetime(u.atoms, r_cut=2.0, pairs=[[0, 1, 2]])
    with pytest.raises(ValueError, match="pairs: a non-empty integer \\(P, 2\\) array"):
        PairLifetime(u.atoms, r_cut=2.0, pairs=[[0.5, 1.0]])
    with pytest.raises(ValueError, match="pairs: atom 7 is not in atomgroup"):
        PairLifetime(u.atoms[[0, 1, 2, 3]], r_cut=2.0, pairs=[[0, 1], [2, 7]])
    with pytest.raises(ValueError, match="pairs: row 1 names an atom twice"):
        PairLifetime(u.atoms, r_cut=2.0, pairs=[[0, 1], [2, 2]])
    with pytest.raises(ValueError, match="needs the periodic box"):
        PairLifetime(ArrayUniverse(positions=x).atoms, r_cut=2.0, device="cpu").run()
    with pytest.raises(_lib.TAError, match="exceeds half the box length"):
        PairLifetime(u.atoms, r_cut=4.5, device="cpu").run()
    with pytest.raises(ValueError, match="invalid dim_type"):
        PairLifetime(u.atoms, r_cut=2.0, dim_type="yx")
    # one device in devices=[...] is one context; keywords given as "not asked for" are accepted
    r = PairLifetime(u.atoms, r_cut=2.0, device="cpu", unwrap=False, compound=None).run().results
    assert r.intermittent.shape == (3,) and r.run_lengths.shape == (4,)
    # an explicit list of atom indices of a subgroup comes back as atom indices
    sub = u.atoms[[1, 4, 5, 8]]
    r = PairLifetime(sub, r_cut=4.0, pairs=[[8, 1], [4, 5]], device="cpu").run().results
    assert r.pairs.tolist() == [[8, 1], [4, 5]]


def class_without_any_bond_gives_nan_with_a_warning(**place):
    x = np.zeros((4, 3, 3))
    x[:, :, 0] = 100.0 * np.arange(3)[None, :]
    with pytest.warns(UserWarning, match="no pair is bonded in any frame"):
        r = PairLifetime(ArrayUniverse(positions=x).atoms, r_cut=1.0, periodic=False, **place).run().results
    assert r.pairs.shape == (0, 2) and np.all(np.isnan(r.intermittent)) and np.all(np.isnan(r.continuous))
    assert np.isnan(r.tau_intermittent) and np.isnan(r.tau_continuous) and np.isnan(r.mean_run) and r.coordination == 0.0
    # an explicit list that is never bonded: the same
    with pytest.warns(UserWarning, match="no pair is bonded in any frame"):
        r = PairLifetime(ArrayUniverse(positions=x).atoms, r_cut=1.0, pairs=[[0, 2]], periodic=False, **place).run().results
    assert r.pairs.tolist() == [[0, 2]] and np.all(np.isnan(r.continuous)) and not r.run_lengths.any()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        x[:, 1, 0] = 0.5
        r = PairLifetime(ArrayUniverse(positions=x).atoms, r_cut=1.0, periodic=False, **place).run().results
    assert r.pairs.tolist() == [[0, 1]] and r.intermittent.tolist() == [1.0] * 4 and r.run_lengths.tolist() == [0, 0, 0, 0, 1]
    assert r.mean_run == 4.0 and r.tau_continuous == 3.0


def test_class_without_any_bond_gives_nan_with_a_warning():
    class_without_any_bond_gives_nan_with_a_warning(device="cpu")


# ---- the C-ABI's argument checks ------------------------------------------------------------------------------------------
def test_argument_checks_with_messages():
    L = _lib.lib()
    n_frames, n_atoms, D = 7, 13, 3
    x = ref.positions(n_frames, n_atoms, D)
    c = cpu_context(x)
    empty = _lib.Context("cpu")
    ia, ib = np.array([0, 2, 5], dtype=np.int64), np.array([1, 3, 12], dtype=np.int64)
    dims = ref.dimensions(ref.BOX, n_frames)
    axes = np.array([0, 1, 2], dtype=np.int32)
    prs = np.array([[0, 1], [2, 12]], dtype=np.int32)
    n_out = ctypes.c_int64(-7)
    ci, runs, nb = np.full(n_frames, -7.0), np.full(n_frames + 1, -7, dtype=np.int64), np.full(n_frames, -7.0)
    buf = np.full((200, 2), -7, dtype=np.int32)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    i64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731
    i32 = lambda *v: np.array(v, dtype=np.int32).reshape(-1, 2)  # noqa: E731

    def find(h=None, n_a=3, a=ia, n_b=3, b=ib, dm=dims, ax=axes, r_cut=1.0, stride=1, out=True):
        return L.ta_pair_find(h or c._h, n_a, p(a), n_b, p(b), p(dm), p(ax), r_cut, stride, ctypes.byref(n_out) if out else None)

    def life(h=None, fft=0, n=2, pr=prs, dm=dims, ax=axes, r_cut=1.0, o_ci=ci, o_runs=runs, o_nb=nb):
        return L.ta_pair_lifetime(h or c._h, fft, n, p(pr), p(dm), p(ax), r_cut, p(o_ci), p(o_runs), p(o_nb))

    def fails(call, code, match, **kw):
        rc = call(**kw)
        assert rc == code, (rc, match, kw)
        msg = L.ta_last_error(kw.get("h") or c._h).decode()
        assert match in msg, (match, msg)
        assert n_out.value == -7 and np.all(ci == -7) and np.all(runs == -7) and np.all(nb == -7) and np.all(buf == -7), \
            "a refused call wrote into an output"

    def boxes(row, frame):
        d = dims.copy()
        d[frame] = row
        return d

    try:
        # ta_pair_find_read before any search
        assert L.ta_pair_find_read(c._h, 200, p(buf)) == -4
        assert "pair_find_read: no pair list has been found" in L.ta_last_error(c._h).decode() and np.all(buf == -7)
        fails(life, -4, "pair_lifetime: no pair list has been found for the staged slab", pr=None)
        # ta_pair_find
        fails(find, -1, "pair_find: the n_pairs output is NULL", out=False)
        fails(find, -1, "pair_find: search_stride must be >= 1", stride=0)
        fails(find, -1, "pair_find: n_a must be >= 1", n_a=0)
        fails(find, -1, "pair_find: n_b must be >= 1", n_b=0)
        for bad in (np.nan, np.inf, 0.0, -0.5):
            fails(find, -1, "pair_find: r_cut must be finite and greater than 0", r_cut=bad)
        fails(find, -1, "pair_find: dimensions without axes", ax=None)
        fails(find, -4, "slabs have not been staged", h=empty._h)
        fails(find, -1, "pair_find: index list a: entry 13 is outside 0 ... n_atoms - 1", a=i64(0, 2, 13))
        fails(find, -1, "pair_find: index list b: entry -1 is outside 0 ... n_atoms - 1", b=i64(-1, 2, 5))
        fails(find, -1, "pair_find: index list a must be strictly increasing", a=i64(0, 2, 2))
        fails(find, -1, "pair_find: index list b must be strictly increasing", b=i64(3, 2, 5))
        fails(find, -1, "pair_find: the index lists overlap (item 2 is in both) but differ: they must be one list or disjoint",
              b=i64(1, 2, 12))
        fails(find, -1, "pair_find: axes: every entry must be 0, 1 or 2", ax=np.array([0, 1, 3], dtype=np.int32))
        fails(find, -1, "box length <= 0", dm=boxes([4.0, 0.0, 8.0, 90, 90, 90], 0))
        fails(find, -1, "pair_find: a non-orthogonal box is not supported (the one-step image is not the minimum image there)",
              dm=boxes([4.0, 2.0, 8.0, 90, 90, 60], 4))
        fails(find, -1, "pair_find: r_cut = 1.100000 exceeds half the box length 2.000000 of frame 0", r_cut=1.1)
        fails(find, -1, "exceeds half the box length 1.500000 of frame 6", dm=boxes([4.0, 1.5, 8.0, 90, 90, 90], 6))
        # ta_pair_lifetime
        fails(life, -1, "fft must be 0 or 1", fft=2)
        fails(life, -1, "pair_lifetime: the ci, runs and nb outputs are all NULL", o_ci=None, o_runs=None, o_nb=None)
        for bad in (np.nan, np.inf, 0.0, -0.5):
            fails(life, -1, "pair_lifetime: r_cut must be finite and greater than 0", r_cut=bad)
        fails(life, -1, "pair_lifetime: dimensions without axes", ax=None)
        fails(life, -4, "slabs have not been staged", h=empty._h)
        fails(life, -1, "pair_lifetime: n_pairs must be 1 ... 2^30 - 1", n=0)
        fails(life, -1, "pair_lifetime: n_pairs must be 1 ... 2^30 - 1", n=2 ** 30)
        fails(life, -1, "pair_lifetime: pair 1 (2, 13) is outside 0 ... n_atoms - 1", pr=i32(0, 1, 2, 13))
        fails(life, -1, "pair_lifetime: pair 0 (-1, 1) is outside 0 ... n_atoms - 1", pr=i32(-1, 1, 2, 12))
        fails(life, -1, "pair_lifetime: pair 1 names item 5 twice", pr=i32(0, 1, 5, 5))
        fails(life, -1, "pair_lifetime: a non-orthogonal box is not supported", dm=boxes([4.0, 2.0, 8.0, 90, 60, 90], 2))
        fails(life, -1, "pair_lifetime: r_cut = 1.100000 exceeds half the box length 2.000000 of frame 0", r_cut=1.1)
        # the boundary: r_cut exactly half the shortest box is accepted, per-frame boxes are, and each output alone is
        assert find(dm=boxes([4.0, 4.0, 8.0, 90, 90, 90], 5)) == 0 and n_out.value >= 0
        n_out.value = -7
        assert life(dm=boxes([4.0, 4.0, 8.0, 90, 90, 90], 5), o_ci=None, o_nb=None) == 0 and np.all(runs >= 0) and np.all(ci == -7)
        runs[:] = -7
        # ta_pair_find_read: the capacity
        assert find(a=None, b=None) == 0
        n = n_out.value
        assert 0 < n < 78
        n_out.value = -7
        assert L.ta_pair_find_read(c._h, n - 1, p(buf)) == -1
        assert f"pair_find_read: capacity {n - 1} is smaller than the {n} pairs found" in L.ta_last_error(c._h).decode()
        assert np.all(buf == -7)
        assert L.ta_pair_find_read(c._h, n, None) == -1 and "pair_find_read: the pairs output is NULL" in L.ta_last_error(c._h).decode()
        assert L.ta_pair_find_read(c._h, 200, p(buf)) == 0 and np.all(buf[:n] >= 0) and np.all(buf[n:] == -7)
        assert np.array_equal(buf[:n], ref.found(x, None, None, np.array(ref.BOX), 1.0, 1))
        # the found list serves ta_pair_lifetime with h_pairs NULL (n_pairs is ignored), until a new staging
        assert life(n=0, pr=None) == 0 and np.array_equal(runs, ref.sums(ref.indicator(x, buf[:n], np.array(ref.BOX), 1.0))[1])
        ci[:], runs[:], nb[:], buf[:] = -7, -7, -7, -7
        # a search that finds nothing leaves an empty list: there is nothing to read, and ta_pair_lifetime refuses it
        assert find(a=i64(0), b=i64(1), n_a=1, n_b=1, dm=None, r_cut=2.0 ** -12) == 0 and n_out.value == 0
        n_out.value = -7
        assert L.ta_pair_find_read(c._h, 200, p(buf)) == -4
        assert "pair_find_read: the found pair list is empty" in L.ta_last_error(c._h).decode() and np.all(buf == -7)
        assert c.pair_find(2.0 ** -12, idx_a=[0], idx_b=[1]).shape == (0, 2)
        fails(life, -4, "pair_lifetime: the found pair list is empty", pr=None)
        (view,) = c.stage_alloc(n_frames, n_atoms, D)
        view[:] = x
        c.stage_commit(0, n_frames)
        fails(life, -4, "pair_lifetime: no pair list has been found for the staged slab", pr=None)
        assert L.ta_pair_find_read(c._h, 200, p(buf)) == -4
        # the wrapper's own checks, and the options
        with pytest.raises(_lib.TAError, match="slabs have not been staged") as e:
            empty.pair_find(1.0)
        assert e.value.code == -4
        with pytest.raises(ValueError, match="expected \\(7, 6\\)"):
            c.pair_find(1.0, dimensions=dims[:3])
        with pytest.raises(ValueError, match="expected an integer \\(n_pairs, 2\\) array"):
            c.pair_lifetime(0, 1.0, np.zeros((3, 3), dtype=np.int32))
        with pytest.raises(_lib.TAError, match="pair_chunk: 0 \\(automatic\\) or the candidate pairs per block"):
            c.set_option("pair_chunk", -1)
        with pytest.raises(_lib.TAError, match="pair_find_chunk: 0 \\(automatic\\) or the searched frames per pass"):
            c.set_option("pair_find_chunk", -1)
    finally:
        c.close()
        empty.close()


def test_tile_and_bitmap_limits():
    """ceil(Na / 256) ceil(Nb / 1024) >= 2^24 and a bitmap above 2^35 bits are refused with messages that name the limits,
    before anything is written: 2.2 million items against themselves; 300000 against the other 300000 (1172 x 293 tiles, 9e10
    bits)"""
    n = 2_200_000
    c = _lib.Context("cpu")
    try:
        c.stage_alloc(1, n, 1, dtype=np.float32)
        c.stage_commit(0, 1)
        with pytest.raises(_lib.TAError, match="pair_find: .* must be below 2\\^24") as e:
            c.pair_find(0.5)
        assert e.value.code == -1
        half = 300_000
        with pytest.raises(_lib.TAError, match="pair_find: the pair bitmap of 300032 x 300032 padded items exceeds 2\\^35 bits") as e:
            c.pair_find(0.5, idx_a=np.arange(half), idx_b=np.arange(half, 2 * half))
        assert e.value.code == -1
    finally:
        c.close()
