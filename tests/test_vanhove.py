"""The self van Hove function (ta_vanhove*, VanHoveSelf) on the CPU backend (Context("cpu"), device="cpu"): closed forms,
the reference of vanhove_ref (counts EQUAL, moments within 1e-10), the argument checks and the class.  (The one return
that needs a slab of 2^31 columns, n_atoms dim >= 2^31, is reached in test_vanhove_shapes.py through ta_vanhove_dev, where
it needs no such slab.)"""
import ctypes

import numpy as np
import pytest

import vanhove_ref as ref
from transport_analysis_amd import VanHoveSelf, _lib, log_lags
from transport_analysis_amd._base import UpdatingAtomGroup
from transport_analysis_amd._mini_mda import ArrayUniverse


def cpu_context(x, dtype=np.float64):
    T, A, D = x.shape
    c = _lib.Context("cpu")
    (view,) = c.stage_alloc(T, A, D, dtype=dtype)
    view[:] = x
    c.stage_commit(0, T)
    return c


def test_ballistic_closed_form():
    """x = x0 + v t on the 1/1024 grid: every pair of atom n at lag tau has r2 = |v_n|^2 tau^2 exactly, so counts[l] is the
    histogram of |v_n| tau_l times (T - tau_l), and alpha2 is the same constant at every lag"""
    rng = np.random.default_rng(3)
    T, A, D = 40, 11, 3
    x0, v = rng.integers(0, 30 * 1024, (A, D)) / 1024.0, rng.integers(-300, 301, (A, D)) / 1024.0
    v[0] = np.array([16, -8, 4]) / 1024.0  # a slow atom: bin 0 at the first lags
    x = x0[None] + v[None] * np.arange(T)[:, None, None]
    lags = ref.lag_sample(T)
    n_bins, dr = 64, 0.125
    v2 = (v * v).sum(axis=1)
    want = np.zeros((len(lags), n_bins + 1), dtype=np.int64)
    for i, tau in enumerate(lags):
        b = np.minimum(np.searchsorted(ref.edges(n_bins, dr), v2 * tau ** 2, side="right") - 1, n_bins)
        want[i] = np.bincount(b, minlength=n_bins + 1) * (T - tau)
    alpha2 = D / (D + 2.0) * np.mean(v2 ** 2) / np.mean(v2) ** 2 - 1.0
    c = cpu_context(x)
    try:
        cnt, mom = c.vanhove(lags, n_bins, dr)
        assert np.array_equal(cnt, want)
        assert want[-1, -1] > 0 and want[1, 0] > 0  # the fastest atoms leave the range, the slowest stay in bin 0
        n = A * (T - lags[1:])
        got = D / (D + 2.0) * (mom[1:, 1] / n) / (mom[1:, 0] / n) ** 2 - 1.0
        assert np.max(np.abs(got - alpha2)) <= 1e-10 * max(1.0, abs(alpha2))
    finally:
        c.close()
    r = VanHoveSelf(ArrayUniverse(positions=x).atoms, lags, r_max=n_bins * dr, n_bins=n_bins, device="cpu").run().results
    assert np.isnan(r.alpha2[0]) and np.max(np.abs(r.alpha2[1:] - alpha2)) <= 1e-10 * max(1.0, abs(alpha2))


def static_atoms(**place):
    x = np.broadcast_to(np.random.default_rng(4).uniform(0, 20, (1, 7, 3)), (12, 7, 3)).copy()
    lags = ref.lag_sample(12)
    r = VanHoveSelf(ArrayUniverse(positions=x).atoms, lags, r_max=2.0, n_bins=10, **place).run().results
    assert np.array_equal(r.counts[:, 0], 7 * (12 - lags)) and not r.counts[:, 1:].any() and not r.overflow.any()
    assert not r.msd.any() and not r.r4.any() and np.all(np.isnan(r.alpha2))


def test_static_atoms():
    static_atoms(device="cpu")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["stage64", "stage32"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_walks_against_reference(D, dtype):
    for T in (1, 2, 3, 7, 65, 200):
        x, lags, refs = ref.case(T, 13, D)
        c = cpu_context(x, dtype)
        try:
            for bins in ref.BINS:
                cnt, mom = c.vanhove(lags, *bins)
                ref.assert_vanhove(cnt, mom, refs[bins], what=f"T={T} bins={bins}")
                # only one output: the same bits
                only = c.vanhove(lags, *bins, moments=False)
                assert only[1] is None and np.array_equal(only[0], cnt)
                only = c.vanhove(lags, *bins, counts=False)
                assert only[0] is None and np.array_equal(only[1], mom)
        finally:
            c.close()


def test_reference_cases_reach_the_edges():
    """what the cases are chosen for: no overflow at small lags, the last real bin and the overflow bin populated at large
    ones, and with the dyadic width pairs exactly on an edge (the <= side of the definition): every pair of lag 0 on e[0],
    and in one dimension, where |d| is a whole number of grid steps, pairs on the edges above it too"""
    x, lags, refs = ref.case(200, 13, 3)
    for bins in ref.BINS:
        cnt = refs[bins][0]
        assert cnt[1, -1] == 0 and cnt[-3:, -1].sum() > 0 and cnt[:, -2].sum() > 0
        assert cnt[0, 0] == 200 * 13
    x, lags, _ = ref.case(200, 13, 1)
    e = ref.edges(64, 0.125)
    on_edge = sum(int(np.isin(((x[tau:] - x[:200 - tau]) ** 2).sum(axis=2), e[1:]).sum()) for tau in lags[1:])
    assert on_edge > 10, on_edge


def test_msd_cross_check():
    """moments[:, 0] / (T - tau) are EinsteinMSD's lag sums (the direct form) at the same lags"""
    x, lags, _ = ref.case(200, 13, 3)
    c = cpu_context(x)
    try:
        _, mom = c.vanhove(lags, 64, 0.125, counts=False)
        ts, _ = c.msd(0)  # the mean over atoms
        got = mom[:, 0] / (200 - lags) / 13
        assert np.max(np.abs(got - ts[lags])) <= 1e-10 * np.max(np.abs(ts[lags]))
    finally:
        c.close()


def test_two_shards_add_up():
    x, lags, refs = ref.case(65, 13, 3)
    bins = ref.BINS[1]
    parts = []
    for lo, hi in ((0, 6), (6, 13)):
        c = cpu_context(x[:, lo:hi])
        try:
            parts.append(c.vanhove(lags, *bins))
        finally:
            c.close()
    ref.assert_vanhove(parts[0][0] + parts[1][0], parts[0][1] + parts[1][1], refs[bins], what="two shards")


def test_threads_do_not_change_the_bits():
    x, lags, _ = ref.case(65, 13, 3)
    runs = []
    for threads in (1, 3):
        c = cpu_context(x)
        try:
            c.set_option("cpu_threads", threads)
            runs.append(c.vanhove(lags, *ref.BINS[0]))
        finally:
            c.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_argument_checks_with_messages():
    L = _lib.lib()
    x, lags, _ = ref.case(7, 13, 3)
    lags = np.ascontiguousarray(lags)
    c = cpu_context(x)
    empty = _lib.Context("cpu")
    cnt, mom = np.empty((len(lags), 11), dtype=np.int64), np.empty((len(lags), 2))
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731

    def fails(code, match, call):
        rc = call()
        assert rc == code, rc
        assert match in L.ta_last_error(c._h).decode() or match in L.ta_last_error(empty._h).decode()

    def call(h=None, n_lags=len(lags), lg=lags, n_bins=10, dr=0.5, o_cnt=cnt, o_mom=mom):
        return L.ta_vanhove(h or c._h, n_lags, None if lg is None else p(lg), n_bins, dr, None if o_cnt is None else p(o_cnt),
                            None if o_mom is None else p(o_mom))

    try:
        assert call() == 0
        before = cnt.copy(), mom.copy()
        fails(-1, "lags are NULL", lambda: call(lg=None))
        fails(-1, "n_lags must be 1 ... 1024", lambda: call(n_lags=0))
        fails(-1, "n_lags must be 1 ... 1024", lambda: call(n_lags=1025))
        fails(-1, "lag -1 is outside", lambda: call(n_lags=2, lg=np.array([-1, 2], dtype=np.int64)))
        fails(-1, "lag 7 is outside", lambda: call(n_lags=2, lg=np.array([1, 7], dtype=np.int64)))
        fails(-1, "strictly increasing", lambda: call(n_lags=3, lg=np.array([1, 3, 3], dtype=np.int64)))
        fails(-1, "strictly increasing", lambda: call(n_lags=3, lg=np.array([1, 3, 2], dtype=np.int64)))
        fails(-1, "n_bins must be 1 ... 4096", lambda: call(n_bins=0))
        fails(-1, "n_bins must be 1 ... 4096", lambda: call(n_bins=4097))
        for dr in (np.nan, np.inf, 0.0, -0.5):
            fails(-1, "dr must be finite and > 0", lambda: call(dr=dr))
        fails(-1, "both NULL", lambda: call(o_cnt=None, o_mom=None))
        # lags are checked before anything is written
        assert np.array_equal(cnt, before[0]) and np.array_equal(mom, before[1])
        fails(-4, "slabs have not been staged", lambda: call(h=empty._h))
        with pytest.raises(_lib.TAError, match="slabs have not been staged") as e:
            empty.vanhove(lags, 10, 0.5)
        assert e.value.code == -4
        with pytest.raises(_lib.TAError, match="both NULL") as e:
            c.vanhove(lags, 10, 0.5, counts=False, moments=False)
        assert e.value.code == -1
        with pytest.raises(ValueError, match="expected \\(n_lags,\\)"):
            c.vanhove(np.ones((2, 2), dtype=np.int64), 10, 0.5)
        with pytest.raises(_lib.TAError, match="vanhove_chunk"):
            c.set_option("vanhove_chunk", -1)
        c.set_option("vanhove_chunk", 2)
    finally:
        c.close()
        empty.close()


def normalisation(**place):
    """sum prob dr + the overflow share = 1, and sum gs V_b likewise, for every d"""
    for dim_type, d in (("xyz", 3), ("xy", 2), ("z", 1)):
        x, lags, _ = ref.case(200, 13, 3)
        v = VanHoveSelf(ArrayUniverse(positions=x).atoms, lags, r_max=5.0, n_bins=50, dim_type=dim_type, **place).run()
        r = v.results
        n_pairs = 13.0 * (200 - lags)
        share = r.overflow / n_pairs
        assert share[1] == 0 and share[-1] > 0
        lo, hi = r.bin_edges[:-1], r.bin_edges[1:]
        shell = {3: 4 * np.pi / 3 * (hi ** 3 - lo ** 3), 2: np.pi * (hi ** 2 - lo ** 2), 1: np.full(50, 2 * v.dr)}[d]
        assert np.max(np.abs((r.prob * v.dr).sum(axis=1) + share - 1.0)) <= 1e-14
        assert np.max(np.abs((r.gs * shell).sum(axis=1) + share - 1.0)) <= 1e-14
        assert r.counts.dtype == np.int64 and r.counts.shape == (len(lags), 50) and r.r.shape == (50,)
        assert np.array_equal(r.counts.sum(axis=1) + r.overflow, n_pairs.astype(np.int64))
        assert np.array_equal(r.times, lags * 1.0) and np.array_equal(r.lags, lags)
        g = v.gaussian_reference()
        with np.errstate(divide="ignore", invalid="ignore"):
            want = (d / (2 * np.pi * r.msd[:, None])) ** (d / 2) * np.exp(-d * r.r[None] ** 2 / (2 * r.msd[:, None]))
        assert g.shape == (len(lags), 50) and np.all(np.isnan(g[0])) and np.allclose(g[1:], want[1:], rtol=1e-13, atol=0)


def test_normalisation():
    normalisation(device="cpu")


def default_lags_are_log_lags(**place):
    assert log_lags(200).tolist() == [1, 2, 3, 4, 6, 7, 10, 13, 18, 24, 32, 42, 56, 75, 100, 133, 178]
    assert log_lags(2).tolist() == [1] and log_lags(1).size == 0 and log_lags(10 ** 6, per_decade=1).tolist() == [1, 10, 100, 1000, 10000, 100000]
    many = log_lags(2 ** 62, per_decade=64)
    assert many.size == 1024 and np.all(np.diff(many) > 0)  # cut at TA_VANHOVE_MAX_LAGS
    x, _, _ = ref.case(200, 13, 3)
    r = VanHoveSelf(ArrayUniverse(positions=x).atoms, r_max=8.0, **place).run().results
    assert np.array_equal(r.lags, log_lags(200)) and r.counts.shape == (17, 200)
    want = ref.reference(x, log_lags(200), 200, 8.0 / 200)
    ref.assert_vanhove(np.column_stack([r.counts, r.overflow]), None, want, what="default lags")


def test_log_lags():
    default_lags_are_log_lags(device="cpu")


def wrapped_walk():
    """a walk on a 1/64 grid and its image in a constant orthorhombic box (both exact in float32)"""
    rng = np.random.default_rng(5)
    box = np.array([16.0, 12.0, 20.0])
    walk = (np.cumsum(rng.integers(-40, 41, size=(120, 9, 3)), axis=0) + 512) / 64.0
    return walk, walk - np.floor(walk / box) * box, box


def unwrap_gives_the_unwrapped_walk(**place):
    walk, wrapped, box = wrapped_walk()
    dims = [*box, 90, 90, 90]
    lags = ref.lag_sample(120)
    kw = dict(r_max=8.0, n_bins=64, **place)
    a = VanHoveSelf(ArrayUniverse(positions=walk).atoms, lags, **kw).run().results
    b = VanHoveSelf(ArrayUniverse(positions=wrapped, dimensions=dims).atoms, lags, unwrap=True, **kw).run().results
    w = VanHoveSelf(ArrayUniverse(positions=wrapped, dimensions=dims).atoms, lags, **kw).run().results
    assert np.array_equal(a.counts, b.counts) and np.array_equal(a.overflow, b.overflow)
    assert not np.array_equal(a.counts, w.counts)  # (the wrapped series is another walk)
    want = ref.reference(walk, lags, 64, 0.125)
    ref.assert_vanhove(np.column_stack([b.counts, b.overflow]), None, want, what="unwrap")
    assert np.max(np.abs(b.msd - a.msd)) <= 1e-10 * np.max(a.msd)


def test_unwrap_gives_the_unwrapped_walk():
    unwrap_gives_the_unwrapped_walk(device="cpu")


def compounds_and_barycentric_frame(**place):
    """16 atoms of equal mass in molecules of 4: the weights 1/4 and 1/16 are dyadic, so the centres (and the centres in the
    barycentric frame) stay on a grid and the counts are exact"""
    x, lags, _ = ref.case(65, 16, 3)
    mol = np.arange(16) // 4
    u = ArrayUniverse(positions=x, masses=np.full(16, 2.0))
    centres = x.reshape(65, 4, 4, 3).mean(axis=2)
    kw = dict(r_max=8.0, n_bins=64, **place)
    r = VanHoveSelf(u.atoms, lags, compound=mol, **kw).run().results
    want = ref.reference(centres, lags, 64, 0.125)
    ref.assert_vanhove(np.column_stack([r.counts, r.overflow]), None, want, what="compound")
    n_pairs = 4.0 * (65 - lags)
    assert np.max(np.abs(r.msd * n_pairs - want[1][:, 0].astype(np.float64))) <= 1e-10 * float(want[1][:, 0].max())
    r = VanHoveSelf(u.atoms, lags, compound=mol, reference_frame="barycentric", **kw).run().results
    want = ref.reference(centres - x.mean(axis=1)[:, None, :], lags, 64, 0.125)
    ref.assert_vanhove(np.column_stack([r.counts, r.overflow]), None, want, what="barycentric")


def test_compounds_and_barycentric_frame():
    compounds_and_barycentric_frame(device="cpu")


def test_class_refusals():
    x, lags, _ = ref.case(7, 13, 3)
    u = ArrayUniverse(positions=x)
    with pytest.raises(TypeError, match="by_particle"):
        VanHoveSelf(u.atoms, lags, r_max=2.0, by_particle=True)
    with pytest.raises(TypeError, match="UpdatingAtomGroup"):
        VanHoveSelf(UpdatingAtomGroup(), lags, r_max=2.0)
    with pytest.raises(TypeError):
        VanHoveSelf(u.atoms, lags)  # r_max is required
    for bad in ([], [1.5, 2.0], [2, 1], [1, 1], [-1, 2], [[1, 2]]):
        with pytest.raises(ValueError, match="lags"):
            VanHoveSelf(u.atoms, bad, r_max=2.0)
    with pytest.raises(ValueError, match="r_max"):
        VanHoveSelf(u.atoms, lags, r_max=0.0)
    with pytest.raises(ValueError, match="n_bins"):
        VanHoveSelf(u.atoms, lags, r_max=2.0, n_bins=4097)
    with pytest.raises(ValueError, match="needs more than the 7 analysed frames"):
        VanHoveSelf(u.atoms, [1, 7], r_max=2.0, device="cpu").run()  # (known at _prepare: before a frame is read)
    with pytest.raises(ValueError, match="at least two analysed frames"):
        VanHoveSelf(ArrayUniverse(positions=x[:1]).atoms, r_max=2.0, device="cpu").run()
    with pytest.raises(ValueError, match="needs the periodic box"):
        VanHoveSelf(u.atoms, lags, r_max=2.0, unwrap=True, device="cpu").run()
    # no box, no volume: accepted without unwrap
    assert VanHoveSelf(u.atoms, lags, r_max=2.0, n_bins=4, device="cpu").run().results.counts.shape == (len(lags), 4)


# ---- the class on several devices and ranks: devices=[...], distributed=True ------------------------------------------------
PLACED_T = 65
INTEGER_KEYS = ("counts",)


def placed_results(A, **place):
    """VanHoveSelf on vanhove_ref.case(65, A, 3) under the placement keywords `place`: {name: array} (placement.py); the
    counts with the overflow column, the moments as the sums the library returns (msd and r4 times the pairs of the lag)"""
    from placement import record_ranges

    x, lags, _ = ref.case(PLACED_T, A, 3)
    out = {}
    for i, (n_bins, dr) in enumerate(ref.BINS):
        r = VanHoveSelf(ArrayUniverse(positions=x).atoms, lags, r_max=n_bins * dr, n_bins=n_bins, **place).run().results
        n_pairs = float(A) * (PLACED_T - lags)
        out["counts" if i == 0 else f"counts_{i}"] = np.column_stack([r.counts, r.overflow])
        out[f"moments_{i}"] = np.stack([r.msd * n_pairs, r.r4 * n_pairs], axis=1)
        record_ranges(out, r)
    return out


def check_placed(out, A, what):
    """placed_results against the reference over ALL atoms: the counts EQUAL, the moments at test_walks_against_reference's bar"""
    _, _, refs = ref.case(PLACED_T, A, 3)
    for i, bins in enumerate(ref.BINS):
        ref.assert_vanhove(out["counts" if i == 0 else f"counts_{i}"], out[f"moments_{i}"], refs[bins], what=f"{what} bins={bins}")


@pytest.mark.parametrize("A", [13, 1])
def test_class_distributed_two_gloo_ranks_cpu_backend(tmp_path, A):
    """A = 13: the ranks hold 6 and 7 atoms; A = 1: rank 0 holds no atom and contributes zeros (_no_moments).  The int64
    counts travel through the all-reduce as float64 and come back as the same integers."""
    import sys

    import placement

    placement.check_ranks(sys.modules[__name__], A, 2, "cpu", tmp_path, dict(device="cpu"))
