"""k_overlap at shapes that reach every branch, through the C-ABI (ta_overlap_staged, ta_overlap_dev, ta_overlap,
ta_group_overlap), GPU only.  Every shape runs on a float64 AND a float32 device slab holding the same values, with lags =
lag_sample(T) and overlap_ref's four cutoffs into a sentinel-filled device array, and asserts: Q EQUAL to overlap_ref's (every
entry, zeros at t0 >= T - lag), k_overlap in the kernel timeline and no widening kernel, repeat runs bit-equal, the staged
slab's bits (padding included) unchanged.

  * the shapes of test_vanhove_shapes (the reads are k_vanhove's): column pairs that straddle atoms (D = 3, odd A), D = 2,
    D = 1 (pairs exactly ON the cutoff 0.5: the strict side); 1, 2, 3 frames with 1 and 2 atoms; an odd frame count over two
    frame blocks (lagged float32 rows at odd and even lags); more atoms than pm_unit_grid gives groups (units loop); eleven
    frame blocks with lags up to T - 1 crossing them;
  * 1, 3 and 4 cutoffs with five lags under "overlap_chunk" 1, 2 and 0: the same bits, and the launches the tile
    (ta_overlap_tile) gives;
  * a smaller call straight after a larger one on the same context; the frame-major entry against the staged one bit for
    bit; two group members on one GPU with an odd split; non-grid float64 values against the CPU backend; the sum over
    origins against ta_vanhove_staged's cumulative counts on the same slab; the class on one device and on two members."""
import numpy as np
import pytest

import overlap_ref as ref
from test_vanhove_shapes import SHAPE_CASES, SLABS, slab_bits, stage, staged_bits, timeline, units_loop_atoms
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu


def run_staged(c, lags, cutoffs, repeat=2):
    """ta_overlap_staged into a sentinel-filled caller buffer, `repeat` times: the runs must agree bit for bit.  -> Q"""
    import torch

    T = c.shape[0]
    runs = []
    for _ in range(repeat):
        q = torch.full((len(np.atleast_1d(cutoffs)), len(lags), T), -7, dtype=torch.int64, device="cuda:0")
        c.overlap_staged(lags, cutoffs, q.data_ptr())
        torch.cuda.synchronize()
        runs.append(q.cpu().numpy())
    for r in runs[1:]:
        assert np.array_equal(runs[0], r), "repeat runs differ"
    return runs[0]


def check(c, dtype, case, what=""):
    x, lags, Q = case[:3]
    got = run_staged(c, lags, ref.CUTOFFS)
    names = timeline(c)
    assert "k_overlap" in names, names
    assert "k_widen_f32" not in names, names  # the slab is read in its own element type
    ref.assert_q(got, Q, lags, what=what)  # (the sentinel is gone everywhere: zeros past the last origin included)
    assert np.array_equal(slab_bits(c, dtype), staged_bits(c, x, dtype)), "the staged slab's bits changed"
    return got


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T,A,D", [pytest.param(*c[1:], id=f"{c[0]}-T{c[1]}-A{c[2]}-D{c[3]}") for c in SHAPE_CASES])
def test_overlap_shapes(T, A, D, dtype):
    case = ref.case(T, A or units_loop_atoms(), D)
    c = stage(_lib.Context(0), case[0], dtype)
    try:
        got = check(c, dtype, case)
        assert np.array_equal(c.overlap(case[1], ref.CUTOFFS), got)  # the host-facing call
    finally:
        c.close()


def launches(n_lags, n_cutoffs, chunk):
    fit = max(1, _lib.overlap_tile() // n_cutoffs)
    per = min(chunk if chunk > 0 else n_lags, n_lags, fit)
    return -(-n_lags // per)


@pytest.mark.parametrize("dtype", SLABS)
def test_overlap_chunks_bit_equal(dtype):
    x, lags, Q, _, _ = ref.case(100, 301, 3)
    pick = [0, 1, 4, 6, 10]  # lags 0, 1, 7, 63, 99
    lags5 = np.ascontiguousarray(lags[pick])
    c = stage(_lib.Context(0), x, dtype)
    try:
        for cuts in ((2, ), (0, 1, 3), (0, 1, 2, 3)):
            cutoffs = [ref.CUTOFFS[i] for i in cuts]
            runs = []
            for chunk in (1, 2, 0):
                c.set_option("overlap_chunk", chunk)
                runs.append(run_staged(c, lags5, cutoffs, repeat=1))
                assert c.kernel_launches("k_overlap") == launches(5, len(cuts), chunk), (cuts, chunk, c.kernel_launches("k_overlap"))
            assert launches(5, len(cuts), 1) == 5
            for r in runs[1:]:
                assert np.array_equal(runs[0], r), cuts
            ref.assert_q(runs[0], Q[list(cuts)][:, pick], lags5, what=f"chunks C={len(cuts)}")
        c.set_option("overlap_chunk", 64)  # more than the tile holds: what it holds
        run_staged(c, lags5, ref.CUTOFFS, repeat=1)
        assert c.kernel_launches("k_overlap") == launches(5, 4, 0)
    finally:
        c.close()


def test_overlap_stale_scratch():
    """A larger call (1101 frames, 300 atoms, 15 lags) then a smaller one (99 frames, 150 atoms, 11 lags) on ONE context
    without ta_trim, through the host-facing call too: its output buffer lies where the first call left values."""
    c = _lib.Context(0)
    try:
        for T, A in ((1101, 300), (99, 150)):
            case = ref.case(T, A, 3)
            stage(c, case[0], np.float64)
            got = check(c, np.float64, case, what=f"T={T}")
            assert np.array_equal(c.overlap(case[1], ref.CUTOFFS), got)
    finally:
        c.close()


def test_overlap_dev_wide_rows():
    """ta_overlap_dev on a frame-major tensor with ld_row > n_atoms dim equals the staged path bit for bit"""
    import torch

    x, lags, Q, _, _ = ref.case(1101, 300, 3)
    T, A, D = x.shape
    ld_row = A * D + 7
    wide = np.full((T, ld_row), 7.5e3)
    wide[:, :A * D] = x.reshape(T, A * D)
    d_x = torch.from_numpy(wide).to("cuda:0")
    c = stage(_lib.Context(0), x, np.float64)
    try:
        want = run_staged(c, lags, ref.CUTOFFS)
        q = torch.full(Q.shape, -7, dtype=torch.int64, device="cuda:0")
        c.overlap_dev(d_x.data_ptr(), T, A, D, ld_row, lags, ref.CUTOFFS, q.data_ptr())
        torch.cuda.synchronize()
        names = timeline(c)
        assert "k_relayout" in names and "k_overlap" in names, names
        assert np.array_equal(want, q.cpu().numpy())
        ref.assert_q(want, Q, lags, what="dev")
    finally:
        c.close()


def test_group_overlap():
    """ta_group_overlap on devices [0, 0] (751 + 750 atoms: an odd split) against one context: the members' Q add up exactly
    -- the sharding property the per-origin output exists for"""
    x, lags, Q, _, _ = ref.case(100, 1501, 3)
    T, A, D = x.shape
    c = stage(_lib.Context(0), x, np.float64)
    g = _lib.Group([0, 0])
    try:
        one = c.overlap(lags, ref.CUTOFFS)
        (views,) = g.stage_alloc(T, A, D)
        assert any((hi - lo) % 2 for lo, hi in g.shards)
        for (lo, hi), view in zip(g.shards, views):
            view[:] = x[:, lo:hi]
        g.stage_commit(0, T)
        got = g.overlap(lags, ref.CUTOFFS)
        assert np.array_equal(got, one)
        ref.assert_q(got, Q, lags, what="group")
    finally:
        g.close()
        c.close()


def test_overlap_gpu_equals_cpu_backend():
    """float64 values off any grid (a walk of normal steps): both backends follow the same r2 arithmetic and the same a2,
    so Q is equal -- no tolerance, no excluded pairs"""
    rng = np.random.default_rng(17)
    T, A, D = 100, 1501, 3
    x = np.cumsum(rng.normal(scale=0.3, size=(T, A, D)), axis=0) + rng.uniform(0, 50, size=(1, A, D))
    lags = ref.lag_sample(T)
    cpu = _lib.Context("cpu")
    c = stage(_lib.Context(0), x, np.float64)
    try:
        (view,) = cpu.stage_alloc(T, A, D, dtype=np.float64)
        view[:] = x
        cpu.stage_commit(0, T)
        want = cpu.overlap(lags, ref.CUTOFFS)
        got = run_staged(c, lags, ref.CUTOFFS)
        assert ref.non_trivial(want, lags, A) >= 8
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    finally:
        c.close()
        cpu.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_overlap_sums_are_vanhove_cumulative_counts(dtype):
    """with a_c = b dr the sum over origins of Q[c, l] is the sum of ta_vanhove_staged's counts[l, :b] on the same slab"""
    import torch

    x, lags, _, _, _ = ref.case(100, 1501, 3)
    n_bins, dr, bs = 64, 0.125, (4, 12, 32)
    c = stage(_lib.Context(0), x, dtype)
    try:
        q = run_staged(c, lags, [b * dr for b in bs], repeat=1)
        cnt = torch.full((len(lags), n_bins + 1), -7, dtype=torch.int64, device="cuda:0")
        c.vanhove_staged(lags, n_bins, dr, cnt.data_ptr(), 0)
        torch.cuda.synchronize()
        cnt = cnt.cpu().numpy()
        for i, b in enumerate(bs):
            assert np.array_equal(q[i].sum(axis=1), cnt[:, :b].sum(axis=1)), b
        assert 0 < q[0].sum() < q[2].sum() < cnt.sum()
    finally:
        c.close()


def test_class_on_two_members_sums_before_the_variance():
    """DynamicSusceptibility on the GPU with float32 staging, on one device and with devices=[0, 0] (751 + 750 atoms): the
    members' Q are added before the variance is taken, so both give the reference's Q, q and chi4 -- the variances of the two
    blocks' own Q would not add up to it"""
    from transport_analysis_amd import DynamicSusceptibility
    from transport_analysis_amd._mini_mda import ArrayUniverse

    x, lags, Q, q, chi4 = ref.case(100, 1501, 3)
    u = ArrayUniverse(positions=x.astype(np.float32))
    ok = (100 - lags) >= 2
    for kw in ({}, {"devices": [0, 0]}):
        r = DynamicSusceptibility(u.atoms, lags, cutoff=ref.CUTOFFS, **kw).run().results
        ref.assert_q(r.overlap_by_origin, Q, lags, what=f"class {kw}")
        err_q = float(np.max(np.abs(r.q - q) / np.where(q > 0, q, 1)))
        err_c = float(np.max(np.abs(r.chi4[:, ok] - chi4[:, ok]) / np.where(chi4[:, ok] > 0, chi4[:, ok], 1)))
        print(f"    class {kw}: q {err_q:.2e}, chi4 {err_c:.2e} relative")
        assert err_q <= 1e-12 and err_c <= 1e-12 and np.all(np.isnan(r.chi4[:, ~ok]))
    halves = [ref.moments(ref.reference(x[:, lo:hi], lags, ref.CUTOFFS)[0], lags, 1501)[1] for lo, hi in ((0, 750), (750, 1501))]
    assert float(np.max(np.abs((halves[0] + halves[1])[:, ok] - chi4[:, ok]))) > 1e-3  # (what summing variances would give)


def test_overlap_dev_refuses_2_pow_31_columns():
    """n_atoms dim >= 2^31: TA_E_INVALID from the frame-major entry before anything is read or written (the pointers are
    those of a small tensor: a call that went on would be caught by the sentinel, not by a fault)"""
    import torch

    d_x = torch.zeros(16, dtype=torch.float64, device="cuda:0")
    q = torch.full((1, 1, 1), -7, dtype=torch.int64, device="cuda:0")
    c = _lib.Context(0)
    try:
        with pytest.raises(_lib.TAError, match="n_atoms \\* dim must be below 2\\^31") as e:
            c.overlap_dev(d_x.data_ptr(), 1, 2 ** 30, 2, 2 ** 31, [0], 0.5, q.data_ptr())
        assert e.value.code == -1
        torch.cuda.synchronize()
        assert bool((q == -7).all())
    finally:
        c.close()
