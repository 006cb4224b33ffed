"""The distinct van Hove function (ta_vanhove_distinct, VanHoveDistinct) on the CPU backend (Context("cpu"), device="cpu"):
the reference of vanhove_distinct_ref (counts EQUAL), closed forms, the argument checks and the class.  (The one return that
needs a slab of 2^31 columns, n_atoms dim >= 2^31, is reached in test_vanhove_distinct_shapes.py on a device-only slab.)"""
import ctypes
import itertools

import numpy as np
import pytest

import vanhove_distinct_ref as ref
from transport_analysis_amd import VanHoveDistinct, _lib
from transport_analysis_amd._base import UpdatingAtomGroup
from transport_analysis_amd._mini_mda import ArrayUniverse


def cpu_context(x, dtype=np.float64):
    T, A, D = x.shape
    c = _lib.Context("cpu")
    (view,) = c.stage_alloc(T, A, D, dtype=dtype)
    view[:] = x
    c.stage_commit(0, T)
    return c


def run_case(c, case, what):
    x, lags, a, b, dims, axes, refs = case
    for bins in ref.BINS:
        got = c.vanhove_distinct(lags, *bins, origin_stride=what[0], idx_a=a, idx_b=b, dimensions=dims, axes=axes)
        ref.assert_counts(got, refs[bins], what=f"{what} bins={bins}")


TS, AS, KINDS = (1, 2, 3, 7, 65), (1, 2, 33), ("same", "disjoint", "overlap")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["stage64", "stage32"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_walks_against_reference(D, dtype):
    """every T x A with the three relations of the index lists, with and without a box, the strides 1, 2, 3, T taken in
    turn; then every T x stride at A = 33 with overlapping lists in a box.  reference() asserts the sum invariant."""
    for T, A in itertools.product(TS, AS):
        c = cpu_context(ref.positions(T, A, D), dtype)
        try:
            for k, (kind, boxed) in enumerate(itertools.product(KINDS, (False, True))):
                stride = (1, 2, 3, T)[(k + T + A) % 4]
                run_case(c, ref.case(T, A, D, stride, kind, boxed), (stride, T, A, kind, boxed))
            if A == 33:
                for stride in (1, 2, 3, T):
                    run_case(c, ref.case(T, A, D, stride, "overlap", True), (stride, T, A, "overlap", True))
        finally:
            c.close()


@pytest.mark.parametrize("D", [1, 2, 3])
def test_per_frame_boxes_at_lag_0(D):
    for T, stride in ((3, 1), (7, 2), (7, 1)):
        c = cpu_context(ref.positions(T, 33, D))
        try:
            run_case(c, ref.case(T, 33, D, stride, "overlap", "frames"), (stride, T, 33, "frames"))
        finally:
            c.close()


def test_reference_cases_reach_the_edges():
    """what the cases are chosen for: pairs in range and in overflow, and with the dyadic width pairs exactly on an edge"""
    x, lags, a, b, dims, axes, refs = ref.case(65, 33, 3, 1, "same", True)
    for bins in ref.BINS:
        assert refs[bins][:, :-1].sum() > 1000 and refs[bins][:, -1].sum() > 1000
    x, lags, a, b, dims, axes, refs = ref.case(65, 33, 1, 1, "same", True)
    e = ref.edges(*ref.BINS[0])
    d = x[0, None, :, 0] - x[0, :, None, 0]
    d = d - np.rint(d / 2.0) * 2.0
    assert int(np.isin(d * d, e[1:]).sum()) > 10


def test_simple_cubic_lattice_at_rest():
    """4^3 sites of spacing 1 in a box of 4, at rest: at every lag the shells r^2 = 1, 2, 3 hold 6, 12, 8 neighbours of every
    site; with dr = 1/4 they sit in bins 4 (exactly on its lower edge), 5 and 6, everything else (r^2 >= 4) is overflow"""
    g = np.arange(4.0)
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + 0.25
    T, N = 5, 64
    x = np.broadcast_to(sites, (T, N, 3)).copy()
    lags, stride = np.array([0, 1, 3]), 2
    c = cpu_context(x)
    try:
        got = c.vanhove_distinct(lags, 8, 0.25, origin_stride=stride, dimensions=ref.dimensions((4.0, 4.0, 4.0), T))
    finally:
        c.close()
    n_orig = ref.n_origins(T, lags, stride)
    assert n_orig.tolist() == [3, 2, 1]
    want = np.zeros((3, 9), dtype=np.int64)
    want[:, 4], want[:, 5], want[:, 6] = 6 * n_orig * N, 12 * n_orig * N, 8 * n_orig * N
    want[:, 8] = (N - 1 - 26) * n_orig * N
    assert np.array_equal(got, want)


def test_two_items_across_the_boundary():
    """0.5 and 7.75 in a box of 8: the image distance 0.75 is the lower edge of bin 3 at dr = 1/4; without the box the
    distance 7.25 is overflow"""
    x = np.zeros((3, 2, 3))
    x[:, 0, 0], x[:, 1, 0] = 0.5, 7.75
    c = cpu_context(x)
    try:
        got = c.vanhove_distinct([0, 2], 16, 0.25, dimensions=ref.dimensions((8.0, 8.0, 8.0), 3))
        want = np.zeros((2, 17), dtype=np.int64)
        want[:, 3] = 2 * 3, 2 * 1
        assert np.array_equal(got, want)
        got = c.vanhove_distinct([0, 2], 16, 0.25)
        assert np.array_equal(got[:, 16], [6, 2]) and not got[:, :16].any()
    finally:
        c.close()


def test_one_item_with_itself_gives_zeros():
    c = cpu_context(ref.positions(7, 5, 3))
    try:
        got = c.vanhove_distinct([0, 1], 10, 0.5, idx_a=[3], idx_b=[3])
        assert got.shape == (2, 11) and not got.any()
    finally:
        c.close()


def test_threads_and_chunks_do_not_change_the_bits():
    """the number of OpenMP threads does not change the counts.  The chunk option is only shown to be ACCEPTED here: it has
    no effect on the CPU backend, which has no scratch to chunk; that forced chunks of 1, 2 and 0 give the same bits is
    checked where it means something, on the GPU (test_vanhove_distinct_shapes.py::test_chunks_bit_equal)"""
    x, lags, a, b, dims, axes, refs = ref.case(65, 33, 3, 2, "overlap", True)
    runs = []
    for threads, chunk in ((1, 0), (3, 0), (2, 1), (2, 2)):
        c = cpu_context(x)
        try:
            c.set_option("cpu_threads", threads)
            c.set_option("vanhove_distinct_chunk", chunk)
            runs.append(c.vanhove_distinct(lags, *ref.BINS[0], origin_stride=2, idx_a=a, idx_b=b, dimensions=dims, axes=axes))
        finally:
            c.close()
    ref.assert_counts(runs[0], refs[ref.BINS[0]])
    assert all(np.array_equal(runs[0], r) for r in runs[1:])


def test_argument_checks_with_messages():
    L = _lib.lib()
    T, A, D = 7, 13, 3
    x = ref.positions(T, A, D)
    c = cpu_context(x)
    empty = _lib.Context("cpu")
    lags = np.array([0, 1, 3], dtype=np.int64)
    ia, ib = np.array([0, 2, 5], dtype=np.int64), np.array([1, 2, 12], dtype=np.int64)
    dims = ref.dimensions(ref.BOX, T)
    axes = np.array([0, 1, 2], dtype=np.int32)
    cnt = np.full((3, 11), -7, dtype=np.int64)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731

    def call(h=None, n_lags=3, lg=lags, stride=1, n_a=3, a=ia, n_b=3, b=ib, dm=dims, ax=axes, n_bins=10, dr=0.1, out=cnt):
        return L.ta_vanhove_distinct(h or c._h, n_lags, p(lg), stride, n_a, p(a), n_b, p(b), p(dm), p(ax), n_bins, dr, p(out))

    def fails(code, match, **kw):
        rc = call(**kw)
        assert rc == code, (rc, kw)
        msg = L.ta_last_error(kw.get("h") or c._h).decode()
        assert match in msg, (match, msg)
        assert np.all(cnt == -7), "a refused call wrote into the output"

    def boxes(row, frame):
        d = dims.copy()
        d[frame] = row
        return d

    i64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731
    try:
        fails(-1, "lags are NULL", lg=None)
        fails(-1, "n_lags must be 1 ... 1024", n_lags=0)
        fails(-1, "n_lags must be 1 ... 1024", n_lags=1025)
        fails(-1, "lag -1 is outside", n_lags=2, lg=i64(-1, 2))
        fails(-1, "lag 7 is outside", n_lags=2, lg=i64(1, 7))
        fails(-1, "strictly increasing", lg=i64(1, 3, 3))
        fails(-1, "strictly increasing", lg=i64(1, 3, 2))
        fails(-1, "n_bins must be 1 ... 4096", n_bins=0)
        fails(-1, "n_bins must be 1 ... 4096", n_bins=4097)
        for dr in (np.nan, np.inf, 0.0, -0.5):
            fails(-1, "dr must be finite and > 0", dr=dr)
        fails(-1, "origin_stride must be >= 1", stride=0)
        fails(-1, "n_a must be >= 1", n_a=0)
        fails(-1, "n_b must be >= 1", n_b=0)
        fails(-1, "index list a: entry 13 is outside", a=i64(0, 2, 13))
        fails(-1, "index list b: entry -1 is outside", b=i64(-1, 2, 5))
        fails(-1, "index list a must be strictly increasing", a=i64(0, 2, 2))
        fails(-1, "index list b must be strictly increasing", b=i64(3, 2, 5))
        fails(-1, "dimensions without axes", ax=None)
        fails(-1, "axes: every entry must be 0, 1 or 2", ax=np.array([0, 1, 3], dtype=np.int32))
        fails(-1, "box length <= 0", dm=boxes([4.0, 0.0, 8.0, 90, 90, 90], 0))
        fails(-1, "non-orthogonal box", dm=boxes([4.0, 2.0, 8.0, 90, 90, 60], 4))  # a triclinic frame, any frame
        fails(-1, "per-frame boxes are accepted only when every lag is 0", dm=boxes([4.0, 4.0, 8.0, 90, 90, 90], 5))
        fails(-1, "exceeds half the box length", n_bins=11)  # r_max = 1.1 > 2 / 2
        fails(-1, "exceeds half the box length 1.5", n_lags=1, lg=i64(0), dm=boxes([4.0, 1.5, 8.0, 90, 90, 90], 6))
        fails(-4, "slabs have not been staged", h=empty._h)
        assert call(out=None) == -1 and "counts output is NULL" in L.ta_last_error(c._h).decode()
        # the boundary: r_max exactly half the shortest box is accepted, and a per-frame box is at lag 0
        assert call() == 0 and np.all(cnt >= 0)
        assert call(n_lags=1, lg=i64(0), dm=boxes([4.0, 4.0, 8.0, 90, 90, 90], 5)) == 0
        with pytest.raises(_lib.TAError, match="slabs have not been staged") as e:
            empty.vanhove_distinct(lags, 10, 0.1)
        assert e.value.code == -4
        with pytest.raises(ValueError, match="expected \\(7, 6\\)"):
            c.vanhove_distinct(lags, 10, 0.1, dimensions=dims[:3])
        with pytest.raises(_lib.TAError, match="vanhove_distinct_chunk"):
            c.set_option("vanhove_distinct_chunk", -1)
    finally:
        c.close()
        empty.close()


def test_only_the_analysed_axes_of_the_box_count():
    """columns on the box axes {0, 2}: a zero length on axis 1 (a slab geometry) is no error, and a length that changes there
    from frame to frame makes no per-frame box, so lags > 0 are accepted; the counts are those of the constant box"""
    x, lags, a, b, dims, axes, refs = ref.case(7, 33, 2, 1, "overlap", True)
    assert axes == (0, 2) and lags[-1] > 0
    flat, moving = dims.copy(), dims.copy()
    flat[:, 1] = 0.0
    moving[:, 1] = 2.0 + np.arange(7)
    c = cpu_context(x)
    try:
        for d in (flat, moving):
            got = c.vanhove_distinct(lags, *ref.BINS[0], idx_a=a, idx_b=b, dimensions=d, axes=axes)
            ref.assert_counts(got, refs[ref.BINS[0]], what="unanalysed axis")
        moving[:, 2] = 8.0 + np.arange(7)  # an analysed axis: a per-frame box
        with pytest.raises(_lib.TAError, match="per-frame boxes are accepted only when every lag is 0"):
            c.vanhove_distinct(lags, *ref.BINS[0], idx_a=a, idx_b=b, dimensions=moving, axes=axes)
    finally:
        c.close()
    u = ArrayUniverse(positions=ref.positions(7, 33, 3), dimensions=[4.0, 2.0, 0.0, 90.0, 90.0, 90.0])
    r = VanHoveDistinct(u.atoms, lags=[0, 1], r_max=1.0, n_bins=64, dim_type="xy", device="cpu").run().results
    want = ref.reference(ref.positions(7, 33, 3)[:, :, :2], [0, 1], 1, None, None, np.array([4.0, 2.0]), 64, 1.0 / 64)
    ref.assert_counts(np.column_stack([r.counts, r.overflow]), want, what="class, slab geometry")
    assert r.rdf is not None and np.all(np.isfinite(r.g))
    with pytest.raises(ValueError, match="box lengths > 0 on the analysed axes"):
        VanHoveDistinct(u.atoms, r_max=1.0, dim_type="xz", device="cpu").run()


def test_tile_count_limit():
    """ceil(Na / 256) ceil(Nb / 1024) >= 2^24 is refused with a message that names the limit, before anything is written:
    2.2 million items on both sides (8594 x 2149 tiles), one frame, one column"""
    A = 2_200_000
    c = _lib.Context("cpu")
    try:
        c.stage_alloc(1, A, 1, dtype=np.float32)
        c.stage_commit(0, 1)
        with pytest.raises(_lib.TAError, match="must be below 2\\^24") as e:
            c.vanhove_distinct([0], 4, 0.5)
        assert e.value.code == -1
        # one side alone may be that long
        got = c.vanhove_distinct([0], 4, 0.5, idx_b=[5])
        assert got.sum() == A - 1 and got[0, 0] == A - 1  # (the slab is zeros: every pair at distance 0)
    finally:
        c.close()


# ---- the class ----------------------------------------------------------------------------------------------------------
def shells(d, edges):
    lo, hi = edges[:-1], edges[1:]
    return {3: 4 * np.pi / 3 * (hi ** 3 - lo ** 3), 2: np.pi * (hi ** 2 - lo ** 2), 1: 2 * (hi - lo)}[d]


def gas(T=8, N=400, box=8.0, seed=0):
    return np.random.default_rng(seed).uniform(0, box, size=(T, N, 3)), [box, box, box, 90.0, 90.0, 90.0]


def class_normalisation(**place):
    """gd, g, rdf and coordination from the counts by the formulas of the class's docstring, to 1e-14, for every d and for two
    groups that overlap"""
    x, lags, _, _, dims, _, _ = ref.case(65, 33, 3, 2, "overlap", True)
    u = ArrayUniverse(positions=x, dimensions=dims[0])
    ga, gb = u.select_atoms("index 0:21"), u.select_atoms("index 11:32")
    for dim_type, d, cols in (("xyz", 3, [0, 1, 2]), ("xz", 2, [0, 2]), ("y", 1, [1])):
        v = VanHoveDistinct(ga, gb, lags, r_max=1.0, n_bins=64, origin_stride=2, dim_type=dim_type, **place).run()
        r = v.results
        want = ref.reference(x[:, 0:33][:, :, cols], lags, 2, np.arange(0, 22), np.arange(11, 33), np.array(ref.BOX)[cols], 64, 1.0 / 64)
        ref.assert_counts(np.column_stack([r.counts, r.overflow]), want, what=f"class {dim_type}")
        n_orig = ref.n_origins(65, lags, 2)
        assert np.array_equal(r.n_origins, n_orig) and np.array_equal(r.lags, lags) and np.array_equal(r.times, lags * 1.0)
        assert np.array_equal(r.counts.sum(axis=1) + r.overflow, n_orig * (22 * 22 - 11))
        gd = r.counts / (n_orig[:, None] * 22.0 * shells(d, r.bin_edges)[None, :])
        rho = (22 * 22 - 11) / (22 * float(np.prod(np.array(ref.BOX)[cols])))
        assert np.max(np.abs(r.gd - gd)) <= 1e-14 * np.max(gd)
        assert np.max(np.abs(r.g - gd / rho)) <= 1e-14 * np.max(gd / rho)
        assert np.array_equal(r.rdf, r.g[0]) and lags[0] == 0
        assert np.max(np.abs(r.coordination - np.cumsum(r.counts[0]) / (n_orig[0] * 22.0))) <= 1e-14 * r.coordination[-1]
        assert r.counts.dtype == np.int64 and r.counts.shape == (len(lags), 64) and r.r.shape == (64,)


def test_class_normalisation():
    class_normalisation(device="cpu")


def class_uniform_gas_has_g_of_one(**place):
    """400 independent uniform points in a box of 8 over 8 frames: the lag-0 g, averaged over the bins with the counts as
    weights, is 1 within 3 / sqrt(the pairs counted), the Poisson error of that many pairs (the reference alone meets it with
    this seed: 1.00063 against a bound of 0.00367)"""
    x, dims = gas()
    r = VanHoveDistinct(ArrayUniverse(positions=x, dimensions=dims).atoms, r_max=4.0, n_bins=64, **place).run().results
    x32 = x.astype(np.float32).astype(np.float64)
    d = x32[:, None, :, :] - x32[:, :, None, :]
    d -= np.rint(d / 8.0) * 8.0
    dist = np.sqrt((d * d).sum(axis=3))[:, ~np.eye(400, dtype=bool)]
    want = np.histogram(dist, bins=r.bin_edges)[0]
    assert np.abs(r.counts[0] - want).sum() <= 4  # (float64 sqrt against squared edges: a pair on an edge may move)
    for counts in (want, r.counts[0]):
        g = counts / (8 * 400.0 * shells(3, r.bin_edges)) / (400 * 399 / (400 * 512.0))
        mean, total = float((g * counts).sum() / counts.sum()), int(counts.sum())
        print(f"    weighted mean of g {mean:.6f}, bound {3 / np.sqrt(total):.6f} ({total} pairs)")
        assert abs(mean - 1.0) <= 3.0 / np.sqrt(total)
    assert np.max(np.abs(r.rdf - g)) <= 1e-14 * np.max(g)
    assert abs(r.coordination[-1] - 399 * (4 * np.pi / 3 * 64) / 512) < 0.5


def test_class_uniform_gas_has_g_of_one():
    class_uniform_gas_has_g_of_one(device="cpu")


def class_same_group_twice_and_no_box(**place):
    x, dims = gas(T=3, N=60)
    u = ArrayUniverse(positions=x, dimensions=dims)
    kw = dict(lags=[0, 1], r_max=3.0, n_bins=30, **place)
    one = VanHoveDistinct(u.atoms, **kw).run().results
    two = VanHoveDistinct(u.atoms, u.atoms, **kw).run().results
    assert np.array_equal(one.counts, two.counts) and np.array_equal(one.overflow, two.overflow)
    assert np.array_equal(one.g, two.g)
    # lags=None: 0 and the logarithmic lags; a lag list without 0 has no rdf
    r = VanHoveDistinct(u.atoms, lags=None, r_max=3.0, n_bins=30, **place).run().results
    assert r.lags.tolist() == [0, 1, 2] and np.array_equal(r.counts[:2], one.counts)
    r = VanHoveDistinct(u.atoms, lags=[1], r_max=3.0, n_bins=30, **place).run().results
    assert r.rdf is None and r.coordination is None and r.g.shape == (1, 30)
    # no periodicity: no box needed, plain distances, and nothing that needs a density
    free = VanHoveDistinct(ArrayUniverse(positions=x).atoms, periodic=False, **kw).run().results
    assert free.g is None and free.rdf is None and free.coordination is None and free.gd.shape == (2, 30)
    assert free.counts.sum() < one.counts.sum()  # (the pairs across the boundary are further apart)
    with pytest.raises(ValueError, match="needs the periodic box"):
        VanHoveDistinct(ArrayUniverse(positions=x).atoms, **kw).run()
    with pytest.raises(_lib.TAError, match="exceeds half the box length"):
        VanHoveDistinct(u.atoms, r_max=4.5, **place).run()


def test_class_same_group_twice_and_no_box():
    class_same_group_twice_and_no_box(device="cpu")


def test_class_refusals():
    x, dims = gas(T=3, N=10)
    u = ArrayUniverse(positions=x, dimensions=dims)
    with pytest.raises(ValueError, match="pair sums cross the shards"):
        VanHoveDistinct(u.atoms, r_max=2.0, devices=[0, 1])
    with pytest.raises(ValueError, match="pair sums cross the blocks"):
        VanHoveDistinct(u.atoms, r_max=2.0, distributed=True)
    with pytest.raises(TypeError, match="compound="):
        VanHoveDistinct(u.atoms, r_max=2.0, compound=np.arange(10) // 2)
    with pytest.raises(TypeError, match="reference_frame="):
        VanHoveDistinct(u.atoms, r_max=2.0, reference_frame="barycentric")
    with pytest.raises(TypeError, match="unwrap="):
        VanHoveDistinct(u.atoms, r_max=2.0, unwrap=True)
    with pytest.raises(TypeError, match="by_particle"):
        VanHoveDistinct(u.atoms, r_max=2.0, by_particle=True)
    with pytest.raises(TypeError, match="UpdatingAtomGroup"):
        VanHoveDistinct(UpdatingAtomGroup(), r_max=2.0)
    with pytest.raises(TypeError, match="UpdatingAtomGroup"):
        VanHoveDistinct(u.atoms, UpdatingAtomGroup(), r_max=2.0)
    with pytest.raises(TypeError):
        VanHoveDistinct(u.atoms)  # r_max is required
    with pytest.raises(ValueError, match="more than once"):
        VanHoveDistinct(u.atoms[[0, 1, 1]], r_max=2.0)
    for bad in ([], [1.5, 2.0], [2, 1], [-1, 2]):
        with pytest.raises(ValueError, match="lags"):
            VanHoveDistinct(u.atoms, lags=bad, r_max=2.0)
    with pytest.raises(ValueError, match="r_max"):
        VanHoveDistinct(u.atoms, r_max=0.0)
    with pytest.raises(ValueError, match="n_bins"):
        VanHoveDistinct(u.atoms, r_max=2.0, n_bins=4097)
    with pytest.raises(ValueError, match="origin_stride"):
        VanHoveDistinct(u.atoms, r_max=2.0, origin_stride=0)
    with pytest.raises(ValueError, match="needs more than the 3 analysed frames"):
        VanHoveDistinct(u.atoms, lags=[0, 3], r_max=2.0, device="cpu").run()
    # one device in devices=[...] is one context
    assert VanHoveDistinct(u.atoms, r_max=2.0, n_bins=4, device="cpu", unwrap=False, compound=None).run().results.counts.shape == (1, 4)


# ---- the class against the reference: the relations of the two groups, the boxes, the origin strides -----------------------
CLASS_CASES = [(kind, boxed, stride) for kind in ("same", "disjoint", "overlap") for boxed in (True, "frames", False) for stride in (1, 3)]
DERIVED_KEYS = ("gd", "g", "rdf", "coordination")


def class_on_case(kind, boxed, stride, **place):
    """VanHoveDistinct on vanhove_distinct_ref.case(65, 33, 3, stride, kind, boxed) under the placement keywords `place`:
    counts, overflow and n_origins EQUAL to the reference's; returns the results (test_classes_gpu.py compares the
    normalised functions with the device="cpu" run's: both come from the same integers through the same NumPy lines)"""
    x, lags, a, b, dims, axes, refs = ref.case(65, 33, 3, stride, kind, boxed)
    u = ArrayUniverse(positions=x, dimensions=dims)
    n_bins, dr = ref.BINS[0]
    v = VanHoveDistinct(u.atoms if a is None else u.atoms[a], None if b is None else u.atoms[b], lags, r_max=n_bins * dr, n_bins=n_bins,
                        origin_stride=stride, periodic=bool(boxed), **place).run()
    r = v.results
    ref.assert_counts(np.column_stack([r.counts, r.overflow]), refs[ref.BINS[0]], what=f"class {kind} box={boxed} stride={stride}")
    assert np.array_equal(r.n_origins, ref.n_origins(65, lags, stride)) and np.array_equal(r.lags, lags)
    assert (r.g is None) == (not boxed) and r.gd.shape == (len(lags), n_bins)
    return r


@pytest.mark.parametrize("kind,boxed,stride", CLASS_CASES)
def test_class_against_reference(kind, boxed, stride):
    class_on_case(kind, boxed, stride, device="cpu")
