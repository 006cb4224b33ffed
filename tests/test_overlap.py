"""The self-overlap per origin and chi_4 (ta_overlap*, DynamicSusceptibility) on the CPU backend (Context("cpu"),
device="cpu"): the C-ABI and every error return, closed forms, the reference of overlap_ref (Q EQUAL), shards, threads and
the class.  (The one return that needs a slab of 2^31 columns, n_atoms dim >= 2^31, is not reached here.)"""
import ctypes

import numpy as np
import pytest

import overlap_ref as ref
from test_vanhove import wrapped_walk
from transport_analysis_amd import DynamicSusceptibility, VanHoveSelf, _lib, log_lags
from transport_analysis_amd._base import UpdatingAtomGroup
from transport_analysis_amd._mini_mda import ArrayUniverse


def cpu_context(x, dtype=np.float64):
    T, A, D = x.shape
    c = _lib.Context("cpu")
    (view,) = c.stage_alloc(T, A, D, dtype=dtype)
    view[:] = x
    c.stage_commit(0, T)
    return c


def test_exports_and_tile():
    assert {"ta_overlap", "ta_overlap_staged", "ta_overlap_dev", "ta_group_overlap", "ta_overlap_tile"} <= set(_lib.EXPORTS)
    assert _lib.overlap_tile() >= 4  # one lag's cutoffs share a launch
    assert _lib.lib().ta_abi_version() == 6


def test_static_atoms():
    x = np.broadcast_to(np.random.default_rng(4).uniform(0, 20, (1, 7, 3)), (12, 7, 3)).copy()
    lags = ref.lag_sample(12)
    r = DynamicSusceptibility(ArrayUniverse(positions=x).atoms, lags, cutoff=(0.25, 1.0), device="cpu").run().results
    Q = r.overlap_by_origin
    assert Q.dtype == np.int64 and Q.shape == (2, len(lags), 12)
    for i, tau in enumerate(lags):
        assert np.all(Q[:, i, :12 - tau] == 7) and not Q[:, i, 12 - tau:].any()
    assert np.array_equal(r.n_origins, 12 - lags)
    assert np.all(r.q == 1.0)
    assert np.all(r.chi4[:, r.n_origins >= 2] == 0.0) and np.all(np.isnan(r.chi4[:, r.n_origins < 2]))


def test_ballistic_step():
    """every atom moves 1/8 per frame along one axis: |d| = tau / 8 for every pair, so Q steps from N to 0 where tau / 8
    reaches a -- and AT a (tau = 4 for a = 0.5: r2 = 0.25 = a2 exactly) the pair is not counted"""
    A, T = 9, 20
    v = np.zeros((A, 3))
    v[np.arange(A), np.arange(A) % 3] = np.where(np.arange(A) % 2, -0.125, 0.125)
    x = np.arange(A * 3).reshape(1, A, 3) / 4.0 + v[None] * np.arange(T)[:, None, None]
    lags = np.array([0, 1, 3, 4, 5, 6, 10], dtype=np.int64)
    for dtype in (np.float64, np.float32):
        c = cpu_context(x, dtype)
        try:
            Q = c.overlap(lags, (0.5, 0.7))
        finally:
            c.close()
        for i, tau in enumerate(lags):
            assert np.all(Q[0, i, :T - tau] == (A if tau < 4 else 0)), (tau, Q[0, i])
            assert np.all(Q[1, i, :T - tau] == (A if tau <= 5 else 0)), (tau, Q[1, i])
            assert not Q[:, i, T - tau:].any()
    r = DynamicSusceptibility(ArrayUniverse(positions=x).atoms, lags, cutoff=(0.5, 0.7), device="cpu").run().results
    assert np.array_equal(r.q[0], (lags < 4).astype(float)) and np.array_equal(r.q[1], (lags <= 5).astype(float))
    assert not r.chi4.any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["stage64", "stage32"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_walks_against_reference(D, dtype):
    for T in (1, 2, 3, 7, 65, 200):
        x, lags, Q, _, _ = ref.case(T, 13, D)
        c = cpu_context(x, dtype)
        try:
            ref.assert_q(c.overlap(lags, ref.CUTOFFS), Q, lags, what=f"T={T} D={D}")
            one = c.overlap(lags, ref.CUTOFFS[2])  # a scalar cutoff: the leading axis stays
            assert one.shape == (1, len(lags), T) and np.array_equal(one[0], Q[2])
        finally:
            c.close()


def test_reference_cases_are_what_they_are_chosen_for():
    """pairs exactly on a = 0.5 in one dimension (the strict side), Q that varies over origins in every dimension"""
    x, lags, Q, _, _ = ref.case(200, 13, 1)
    assert ref.reference(x, lags, ref.CUTOFFS)[1][0] >= 1
    for D in (1, 2, 3):
        x, lags, Q, q, chi4 = ref.case(200, 13, D)
        assert ref.non_trivial(Q, lags, 13) >= 8
        assert q[0, 0] == 1 and chi4[0, 0] == 0  # lag 0: every atom overlaps itself


def test_two_shards_add_up():
    x, lags, Q, _, _ = ref.case(65, 13, 3)
    parts = []
    for lo, hi in ((0, 6), (6, 13)):
        c = cpu_context(x[:, lo:hi])
        try:
            parts.append(c.overlap(lags, ref.CUTOFFS))
        finally:
            c.close()
    ref.assert_q(parts[0] + parts[1], Q, lags, what="two shards")
    assert (parts[0] != Q).any()


def test_threads_do_not_change_the_bits():
    x, lags, Q, _, _ = ref.case(65, 13, 3)
    runs = []
    for threads in (1, 4):
        c = cpu_context(x)
        try:
            c.set_option("cpu_threads", threads)
            runs.append(c.overlap(lags, ref.CUTOFFS))
        finally:
            c.close()
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], Q)


def test_argument_checks_with_messages():
    L = _lib.lib()
    x, lags, _, _, _ = ref.case(7, 13, 3)
    lags = np.ascontiguousarray(lags)
    cut = np.array([0.5, 0.7])
    c = cpu_context(x)
    empty = _lib.Context("cpu")
    q = np.full((2, len(lags), 7), -7, dtype=np.int64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731

    def fails(code, match, call):
        rc = call()
        assert rc == code, rc
        assert match in L.ta_last_error(c._h).decode() or match in L.ta_last_error(empty._h).decode(), L.ta_last_error(c._h)

    def call(h=None, n_lags=len(lags), lg=lags, n_cut=2, cu=cut, out=q):
        return L.ta_overlap(h or c._h, n_lags, None if lg is None else p(lg), n_cut, None if cu is None else p(cu),
                            None if out is None else p(out))

    i64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731
    try:
        fails(-1, "overlap: lags are NULL", lambda: call(lg=None))
        fails(-1, "overlap: n_lags must be 1 ... 1024", lambda: call(n_lags=0))
        fails(-1, "overlap: n_lags must be 1 ... 1024", lambda: call(n_lags=1025))
        fails(-1, "overlap: cutoffs are NULL", lambda: call(cu=None))
        fails(-1, "overlap: n_cutoffs must be 1 ... 4", lambda: call(n_cut=0))
        fails(-1, "overlap: n_cutoffs must be 1 ... 4", lambda: call(n_cut=5, cu=np.arange(1.0, 6.0)))
        for bad in (np.nan, np.inf, 0.0, -0.5):
            fails(-1, "overlap: cutoff 1 must be finite and > 0", lambda: call(cu=np.array([0.5, bad])))
        fails(-1, "overlap: the cutoffs must be strictly increasing", lambda: call(cu=np.array([0.5, 0.5])))
        fails(-1, "overlap: the cutoffs must be strictly increasing", lambda: call(cu=np.array([0.7, 0.5])))
        fails(-1, "overlap: the output is NULL", lambda: call(out=None))
        fails(-1, "overlap: lag -1 is outside", lambda: call(n_lags=2, lg=i64(-1, 2)))
        fails(-1, "overlap: lag 7 is outside", lambda: call(n_lags=2, lg=i64(1, 7)))
        fails(-1, "overlap: the lags must be strictly increasing", lambda: call(n_lags=3, lg=i64(1, 3, 3)))
        fails(-1, "overlap: the lags must be strictly increasing", lambda: call(n_lags=3, lg=i64(1, 3, 2)))
        # a rejected call writes nothing
        assert np.all(q == -7)
        fails(-4, "slabs have not been staged", lambda: call(h=empty._h))
        assert np.all(q == -7)
        assert call() == 0 and not np.any(q == -7)
        with pytest.raises(_lib.TAError, match="slabs have not been staged") as e:
            empty.overlap(lags, cut)
        assert e.value.code == -4
        with pytest.raises(ValueError, match="expected \\(n_lags,\\)"):
            c.overlap(np.ones((2, 2), dtype=np.int64), cut)
        with pytest.raises(ValueError, match="cutoffs: shape"):
            c.overlap(lags, np.ones((2, 2)))
        with pytest.raises(_lib.TAError, match="overlap_chunk"):
            c.set_option("overlap_chunk", -1)
        c.set_option("overlap_chunk", 2)
    finally:
        c.close()
        empty.close()


def test_output_bound():
    """n_cutoffs n_lags n_frames > 2^27 is refused before anything is written; at the bound's own side the call runs"""
    L = _lib.lib()
    T = 2 ** 15 + 8
    c = cpu_context(np.zeros((T, 1, 1)))
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    try:
        lags = np.arange(1024, dtype=np.int64)
        cut = np.array(ref.CUTOFFS)
        q = np.full(8, -7, dtype=np.int64)
        assert 4 * 1024 * T > 2 ** 27
        assert L.ta_overlap(c._h, 1024, p(lags), 4, p(cut), p(q)) == -1
        msg = L.ta_last_error(c._h).decode()
        assert "exceeds 2^27" in msg and str(4 * 1024 * T) in msg, msg
        assert np.all(q == -7)
        assert c.overlap(lags[:2], cut[:1]).shape == (1, 2, T)
    finally:
        c.close()


# ---- the class ---------------------------------------------------------------------------------------------------------
def class_against_reference(**place):
    for D, dim_type in ((3, "xyz"), (2, "xy"), (1, "x")):
        x3 = ref.walk(200, 13, 3, 1)
        x = x3[:, :, :D]
        lags = ref.lag_sample(200)
        Q, _ = ref.reference(x, lags, ref.CUTOFFS)
        q, chi4 = ref.moments(Q, lags, 13)
        r = DynamicSusceptibility(ArrayUniverse(positions=x3).atoms, lags, cutoff=ref.CUTOFFS, dim_type=dim_type, **place).run().results
        ref.assert_q(r.overlap_by_origin, Q, lags, what=f"class {dim_type}")
        assert np.array_equal(r.lags, lags) and np.array_equal(r.times, lags * 1.0) and np.array_equal(r.cutoffs, ref.CUTOFFS)
        assert np.array_equal(r.n_origins, 200 - lags)
        assert r.q.shape == r.chi4.shape == (4, len(lags)) and r.chi4.dtype == np.float64
        err_q = float(np.max(np.abs(r.q - q) / np.where(q > 0, q, 1)))
        ok = r.n_origins >= 2
        assert ok.sum() == len(lags) - 1 and np.all(np.isnan(r.chi4[:, ~ok]))  # lag T - 1: one origin
        err_c = float(np.max(np.abs(r.chi4[:, ok] - chi4[:, ok]) / np.where(chi4[:, ok] > 0, chi4[:, ok], 1)))
        print(f"    {dim_type}: q {err_q:.2e}, chi4 {err_c:.2e} relative")
        assert err_q <= 1e-12 and err_c <= 1e-12
        assert float(chi4[:, ok].max()) > 0


def test_class_against_reference():
    class_against_reference(device="cpu")


def class_scalar_cutoff_and_default_lags(**place):
    x, _, _, _, _ = ref.case(200, 13, 3)
    r = DynamicSusceptibility(ArrayUniverse(positions=x).atoms, cutoff=1.5, **place).run().results
    lags = log_lags(200)
    assert np.array_equal(r.lags, lags)
    assert r.overlap_by_origin.shape == (1, len(lags), 200) and r.q.shape == r.chi4.shape == (1, len(lags))
    Q, _ = ref.reference(x, lags, (1.5,))
    ref.assert_q(r.overlap_by_origin, Q, lags, what="scalar cutoff")


def test_class_scalar_cutoff_and_default_lags():
    class_scalar_cutoff_and_default_lags(device="cpu")


def class_float32_staging_is_the_same(**place):
    x, lags, Q, _, _ = ref.case(65, 13, 3)
    u = ArrayUniverse(positions=x.astype(np.float32))
    r = DynamicSusceptibility(u.atoms, lags, cutoff=ref.CUTOFFS, **place).run().results
    ref.assert_q(r.overlap_by_origin, Q, lags, what="float32 staging")


def test_class_float32_staging_is_the_same():
    class_float32_staging_is_the_same(device="cpu")


def unwrap_gives_the_unwrapped_walk(**place):
    walk, wrapped, box = wrapped_walk()
    dims = [*box, 90, 90, 90]
    lags = ref.lag_sample(120)
    kw = dict(cutoff=(0.5, 1.5, 4.0), **place)
    a = DynamicSusceptibility(ArrayUniverse(positions=walk).atoms, lags, **kw).run().results
    b = DynamicSusceptibility(ArrayUniverse(positions=wrapped, dimensions=dims).atoms, lags, unwrap=True, **kw).run().results
    w = DynamicSusceptibility(ArrayUniverse(positions=wrapped, dimensions=dims).atoms, lags, **kw).run().results
    assert np.array_equal(a.overlap_by_origin, b.overlap_by_origin)
    assert not np.array_equal(a.overlap_by_origin, w.overlap_by_origin)  # (the wrapped series is another walk)
    ref.assert_q(b.overlap_by_origin, ref.reference(walk, lags, (0.5, 1.5, 4.0))[0], lags, what="unwrap")
    assert np.array_equal(a.chi4, b.chi4, equal_nan=True)


def test_unwrap_gives_the_unwrapped_walk():
    unwrap_gives_the_unwrapped_walk(device="cpu")


def compounds_with_dyadic_weights(**place):
    """16 atoms of equal mass in molecules of 4: the weights 1/4 and 1/16 are dyadic, so the centres (and the centres in the
    barycentric frame) stay on a grid and Q is exact; N is the number of compounds"""
    x, lags, _, _, _ = ref.case(65, 16, 3)
    mol = np.arange(16) // 4
    u = ArrayUniverse(positions=x, masses=np.full(16, 2.0))
    centres = x.reshape(65, 4, 4, 3).mean(axis=2)
    kw = dict(cutoff=ref.CUTOFFS, **place)
    r = DynamicSusceptibility(u.atoms, lags, compound=mol, **kw).run().results
    Q, _ = ref.reference(centres, lags, ref.CUTOFFS)
    ref.assert_q(r.overlap_by_origin, Q, lags, what="compound")
    q, _ = ref.moments(Q, lags, 4)
    assert np.max(np.abs(r.q - q)) <= 1e-12 and r.q[0, 0] == 1.0
    r = DynamicSusceptibility(u.atoms, lags, compound=mol, reference_frame="barycentric", **kw).run().results
    Q, _ = ref.reference(centres - x.mean(axis=1)[:, None, :], lags, ref.CUTOFFS)
    ref.assert_q(r.overlap_by_origin, Q, lags, what="barycentric")


def test_compounds_with_dyadic_weights():
    compounds_with_dyadic_weights(device="cpu")


def test_cumulative_counts_of_vanhove_self():
    """with a = b dr the sum of Q over origins is the cumulative count of VanHoveSelf's bins below b, exactly"""
    x, lags, _, _, _ = ref.case(200, 13, 3)
    u = ArrayUniverse(positions=x)
    v = VanHoveSelf(u.atoms, lags, r_max=8.0, n_bins=64, device="cpu").run().results
    r = DynamicSusceptibility(u.atoms, lags, cutoff=(0.5, 1.5, 4.0), device="cpu").run().results
    for c, b in enumerate((4, 12, 32)):
        assert v.bin_edges[b] == r.cutoffs[c]
        assert np.array_equal(r.overlap_by_origin[c].sum(axis=1), v.counts[:, :b].sum(axis=1))
    assert 0 < r.overlap_by_origin[0].sum() < r.overlap_by_origin[2].sum()


def test_class_refusals():
    x, lags, _, _, _ = ref.case(7, 13, 3)
    u = ArrayUniverse(positions=x)
    with pytest.raises(TypeError, match="by_particle"):
        DynamicSusceptibility(u.atoms, lags, cutoff=1.0, by_particle=True)
    with pytest.raises(TypeError, match="UpdatingAtomGroup"):
        DynamicSusceptibility(UpdatingAtomGroup(), lags, cutoff=1.0)
    with pytest.raises(TypeError):
        DynamicSusceptibility(u.atoms, lags)  # cutoff is required
    for bad in ([], [1.5, 2.0], [2, 1], [1, 1], [-1, 2], [[1, 2]]):
        with pytest.raises(ValueError, match="lags"):
            DynamicSusceptibility(u.atoms, bad, cutoff=1.0)
    for bad in ([], [1, 2, 3, 4, 5], 0.0, -1.0, np.nan, np.inf, [2.0, 1.0], [1.0, 1.0], [[1.0, 2.0]]):
        with pytest.raises(ValueError, match="cutoff"):
            DynamicSusceptibility(u.atoms, lags, cutoff=bad)
    with pytest.raises(ValueError, match="needs more than the 7 analysed frames"):
        DynamicSusceptibility(u.atoms, [1, 7], cutoff=1.0, device="cpu").run()
    with pytest.raises(ValueError, match="at least two analysed frames"):
        DynamicSusceptibility(ArrayUniverse(positions=x[:1]).atoms, cutoff=1.0, device="cpu").run()
    with pytest.raises(ValueError, match="needs the periodic box"):
        DynamicSusceptibility(u.atoms, lags, cutoff=1.0, unwrap=True, device="cpu").run()
    doc = DynamicSusceptibility.__doc__
    assert "ensemble-dependent" in doc and "origins are correlated" in doc


# ---- the class on several devices and ranks: devices=[...], distributed=True ------------------------------------------------
PLACED_T = 65
INTEGER_KEYS = ("Q",)


def placed_results(A, **place):
    """DynamicSusceptibility on overlap_ref.case(65, A, 3) under the placement keywords `place`: {name: array} (placement.py)"""
    from placement import record_ranges

    x, lags, _, _, _ = ref.case(PLACED_T, A, 3)
    r = DynamicSusceptibility(ArrayUniverse(positions=x).atoms, lags, cutoff=ref.CUTOFFS, **place).run().results
    out = {"Q": r.overlap_by_origin, "q": r.q, "chi4": r.chi4}
    record_ranges(out, r)
    return out


def check_placed(out, A, what):
    """placed_results against the reference over ALL atoms: Q EQUAL, q and chi4 at test_class_against_reference's bar.  The
    blocks' Q are added before the variance is taken: the blocks' own variances would not add up to chi4 (asserted for
    devices=[0, 0] in test_overlap_shapes.py)"""
    x, lags, Q, q, chi4 = ref.case(PLACED_T, A, 3)
    ref.assert_q(out["Q"], Q, lags, what=what)
    ok = (PLACED_T - lags) >= 2
    err_q = float(np.max(np.abs(out["q"] - q) / np.where(q > 0, q, 1)))
    err_c = float(np.max(np.abs(out["chi4"][:, ok] - chi4[:, ok]) / np.where(chi4[:, ok] > 0, chi4[:, ok], 1)))
    print(f"    {what}: q {err_q:.2e}, chi4 {err_c:.2e} relative")
    assert err_q <= 1e-12 and err_c <= 1e-12 and np.all(np.isnan(out["chi4"][:, ~ok]))


@pytest.mark.parametrize("A", [13, 1])
def test_class_distributed_two_gloo_ranks_cpu_backend(tmp_path, A):
    """A = 13: the ranks hold 6 and 7 atoms; A = 1: rank 0 holds no atom and contributes zeros (_no_moments).  The int64 Q
    travels through the all-reduce as float64 and comes back as the same integers, and the variance is taken of the sum."""
    import sys

    import placement

    placement.check_ranks(sys.modules[__name__], A, 2, "cpu", tmp_path, dict(device="cpu"))
    if A > 1:
        x, lags, _, _, chi4 = ref.case(PLACED_T, A, 3)
        ok = (PLACED_T - lags) >= 2
        halves = [ref.moments(ref.reference(x[:, lo:hi], lags, ref.CUTOFFS)[0], lags, A)[1] for lo, hi in ((0, A // 2), (A // 2, A))]
        assert float(np.max(np.abs((halves[0] + halves[1])[:, ok] - chi4[:, ok]))) > 1e-3  # (what summing variances would give)
