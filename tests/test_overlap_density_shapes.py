"""k_overlap_density at shapes that reach every branch, through the C-ABI (ta_overlap_density_staged, ta_overlap_density,
ta_group_overlap_density), GPU only.  Every shape of test_vanhove_shapes (the reads are k_vanhove's) runs on a float64 AND a
float32 device slab holding the same values, with lags = lag_sample(T), overlap_ref's four cutoffs and overlap_density_ref's
five wavevectors (k = 0 the last: three launches per chunk of lags, the last with one wavevector) into a sentinel-filled device
array, and asserts: W within overlap_density_ref's bar per entry, +0.0 at t0 >= T - lag, k_overlap_density in the kernel
timeline and no widening kernel, repeat runs bit-equal, the staged slab's bits (padding included) unchanged, the host-facing
call bit-equal to the staged one.

  * column pairs that straddle atoms (D = 3, odd A), D = 2, D = 1; 1, 2, 3 frames with 1 and 2 atoms; an odd frame count over
    several frame blocks (lagged float32 rows at odd and even lags); more atoms than the launch has groups (units loop);
    10300 frames with lags up to T - 1 crossing the blocks;
  * the wavevector tail K = 1, KC, KC + 1, 2 KC + 1 with the launches the tile (ta_overlap_density_tile) gives;
  * 1, 3 and 4 cutoffs with five lags under "overlap_density_chunk" 1, 2, 0 and 64: the same bits, and the predicted
    launches (a shorter last launch among them);
  * a smaller call straight after a larger one on the same context; non-grid float64 values against the CPU backend within
    the sum of both bars; with a cutoff that takes every atom in, W[j, ., l, t0] against ta_partial_density_staged's density
    at t0 within the two density bars; 2^31 columns refused."""
import numpy as np
import pytest

import overlap_density_ref as ref
import scatter_ref
from test_vanhove_shapes import SHAPE_CASES, SLABS, slab_bits, stage, staged_bits, timeline, units_loop_atoms
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu


def run_staged(c, k, lags, cutoffs, repeat=2):
    """ta_overlap_density_staged into a sentinel-filled caller buffer, `repeat` times: the runs must agree bit for bit.
    -> W float64 (K, C, L, T, 2)"""
    import torch

    T = c.shape[0]
    runs = []
    for _ in range(repeat):
        w = torch.full((len(k), len(np.atleast_1d(cutoffs)), len(lags), T, 2), -7.5, dtype=torch.float64, device="cuda:0")
        c.overlap_density_staged(k, lags, cutoffs, w.data_ptr())
        torch.cuda.synchronize()
        runs.append(w.cpu().numpy())
    for r in runs[1:]:
        assert np.array_equal(runs[0].view(np.uint64), r.view(np.uint64)), "repeat runs differ"
    return runs[0]


def check(c, dtype, case, what=""):
    x, k, lags = case[:3]
    got = run_staged(c, k, lags, ref.CUTOFFS)
    names = timeline(c)
    assert "k_overlap_density" in names and "k_overlap_density_sum" in names, names
    assert "k_widen_f32" not in names, names  # the slab is read in its own element type
    ref.assert_w(got, case, what=what)  # (the sentinel is gone everywhere: +0.0 past the last origin included)
    assert np.array_equal(slab_bits(c, dtype), staged_bits(c, x, dtype)), "the staged slab's bits changed"
    return got


def launches(n_k, n_lags, n_cutoffs, chunk=0):
    tile = _lib.overlap_density_tile()
    fit = max(1, tile["SL"] // n_cutoffs)
    per = min(chunk if chunk > 0 else n_lags, n_lags, fit)
    return -(-n_k // tile["KC"]) * -(-n_lags // per)


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T,A,D", [pytest.param(*c[1:], id=f"{c[0]}-T{c[1]}-A{c[2]}-D{c[3]}") for c in SHAPE_CASES])
def test_overlap_density_shapes(T, A, D, dtype):
    case = ref.case(T, A or units_loop_atoms(), D)
    c = stage(_lib.Context(0), case[0], dtype)
    try:
        got = check(c, dtype, case)
        assert c.kernel_launches("k_overlap_density") == launches(5, len(case[2]), 4)
        host = ref.as_parts(c.overlap_density(case[1], case[2], ref.CUTOFFS))  # the host-facing call
        assert np.array_equal(host.view(np.uint64), got.view(np.uint64))
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_wavevector_tail(dtype):
    case = ref.case(100, 301, 3)
    x, k, lags = case[:3]
    KC = _lib.overlap_density_tile()["KC"]
    c = stage(_lib.Context(0), x, dtype)
    try:
        full = run_staged(c, k, lags, ref.CUTOFFS, repeat=1)
        for K in (1, KC, KC + 1, 2 * KC + 1):
            assert K <= len(k)
            got = run_staged(c, k[:K], lags, ref.CUTOFFS, repeat=1)
            assert c.kernel_launches("k_overlap_density") == launches(K, len(lags), 4), K
            assert c.kernel_launches("k_overlap_density_sum") == launches(K, len(lags), 4), K
            assert np.array_equal(got.view(np.uint64), full[:K].view(np.uint64)), K  # (a wavevector's bits do not depend on its launch)
        ref.assert_w(full, case, what="tail")
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_chunks_bit_equal(dtype):
    case = ref.case(100, 301, 3)
    x, k, lags = case[:3]
    pick = [0, 1, 4, 6, 10]  # lags 0, 1, 7, 63, 99
    lags5 = np.ascontiguousarray(lags[pick])
    c = stage(_lib.Context(0), x, dtype)
    try:
        for cuts in ((2, ), (0, 1, 3), (0, 1, 2, 3)):
            cutoffs = [ref.CUTOFFS[i] for i in cuts]
            runs = []
            for chunk in (1, 2, 0, 64):
                c.set_option("overlap_density_chunk", chunk)
                runs.append(run_staged(c, k, lags5, cutoffs, repeat=1))
                n = c.kernel_launches("k_overlap_density")
                assert n == launches(5, 5, len(cuts), chunk), (cuts, chunk, n)
            # five lags: C = 1 takes 4 + 1 (a shorter last launch), C = 3 and 4 one lag per launch
            assert launches(5, 5, 1) == 3 * 2 and launches(5, 5, 1, 2) == 3 * 3 and launches(5, 5, 3) == launches(5, 5, 4) == 3 * 5
            for r in runs[1:]:
                assert np.array_equal(runs[0].view(np.uint64), r.view(np.uint64)), cuts
            ref.assert_w(runs[0], case, what=f"chunks C={len(cuts)}", pick=(np.arange(5), list(cuts), pick))
    finally:
        c.close()


def test_stale_scratch():
    """A larger call (1101 frames, 300 atoms) then a smaller one (99 frames, 150 atoms) on ONE context without ta_trim, through
    the host-facing call too: the partials and the output buffer lie where the first call left values."""
    c = _lib.Context(0)
    try:
        for T, A in ((1101, 300), (99, 150)):
            case = ref.case(T, A, 3)
            stage(c, case[0], np.float64)
            got = check(c, np.float64, case, what=f"T={T}")
            host = ref.as_parts(c.overlap_density(case[1], case[2], ref.CUTOFFS))
            assert np.array_equal(host.view(np.uint64), got.view(np.uint64))
    finally:
        c.close()


def test_gpu_against_the_cpu_backend():
    """float64 values off any grid (a walk of normal steps): both backends follow the same r2 arithmetic and the same a2, so
    the indicator is the same, and the same phase expression: each is within its bar of the exact sum, so they are within
    the sum of both bars of each other (the CPU backend's Q is the entry's count)"""
    rng = np.random.default_rng(17)
    T, A, D = 100, 1501, 3
    x = np.cumsum(rng.normal(scale=0.3, size=(T, A, D)), axis=0) + rng.uniform(0, 50, size=(1, A, D))
    lags = ref.lag_sample(T)
    k = ref.wavevectors(5, D)
    cpu = _lib.Context("cpu")
    c = stage(_lib.Context(0), x, np.float64)
    try:
        (view,) = cpu.stage_alloc(T, A, D, dtype=np.float64)
        view[:] = x
        cpu.stage_commit(0, T)
        want = ref.as_parts(cpu.overlap_density(k, lags, ref.CUTOFFS))
        Q = cpu.overlap(lags, ref.CUTOFFS)
        got = run_staged(c, k, lags, ref.CUTOFFS)
        bar = 2 * ref.bar(x, k, Q)
        err = np.max(np.abs(got - want), axis=4)
        ratio = float(np.max(np.where(bar[None] > 0, err / np.where(bar[None] > 0, bar[None], 1.0), 0.0)))
        print(f"    gpu - cpu: worst difference / (sum of both bars) {ratio:.3f}")
        assert np.all(err <= bar[None]), np.argwhere(err > bar[None])[:5]
        assert np.array_equal(got[-1, ..., 0], Q) and not got[-1, ..., 1].any()  # k = 0: the same counts on both
        assert int(np.count_nonzero((Q > 0) & (Q < A))) > 100
    finally:
        c.close()
        cpu.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_everyone_inside_is_the_density(dtype):
    """a cutoff that takes every atom in at every lag: W[j, 0, l, t0] is the plain density of frame t0, the one
    ta_partial_density_staged forms with one species -- each within scatter_ref.density_bar of the exact one"""
    import torch

    x, k, lags = ref.case(100, 301, 3)[:3]
    T, A, _ = x.shape
    huge = 1e6
    c = stage(_lib.Context(0), x, dtype)
    try:
        w = run_staged(c, k, lags, huge, repeat=1)
        rho = torch.full((len(k), 1, T, 2), -7.5, dtype=torch.float64, device="cuda:0")
        lab = torch.zeros(A, dtype=torch.int32, device="cuda:0")
        c.partial_density_staged(0, k, 1, lab.data_ptr(), rho.data_ptr())
        torch.cuda.synchronize()
        rho = rho.cpu().numpy()[:, 0]  # (K, T, 2)
        bar = 2 * scatter_ref.density_bar(x, k)
        worst = 0.0
        for i, tau in enumerate(int(t) for t in lags):
            err = float(np.max(np.abs(w[:, 0, i, :T - tau] - rho[:, :T - tau])))
            worst = max(worst, err)
            assert err <= bar, (tau, err, bar)
            assert not w[:, 0, i, T - tau:].any()
        print(f"    W - density: {worst:.3e} (bar {bar:.3e})")
    finally:
        c.close()


def test_group_on_one_gpu_with_an_odd_split():
    """ta_group_overlap_density on devices [0, 0] (751 + 750 atoms): the members' W add up to the reference within its bar
    and one more rounding -- the sharding property the per-origin output exists for"""
    case = ref.case(100, 1501, 3)
    x, k, lags = case[:3]
    T, A, D = x.shape
    g = _lib.Group([0, 0])
    try:
        (views,) = g.stage_alloc(T, A, D)
        assert any((hi - lo) % 2 for lo, hi in g.shards)
        for (lo, hi), view in zip(g.shards, views):
            view[:] = x[:, lo:hi]
        g.stage_commit(0, T)
        ref.assert_w(g.overlap_density(k, lags, ref.CUTOFFS), case, what="group", extra_bar=A * ref.U_R)
    finally:
        g.close()


def test_class_on_two_members_sums_before_anything_is_squared():
    """FourPointStructureFactor on the GPU with float32 staging, on one device and with devices=[0, 0] (751 + 750 atoms): the
    members' W are added before anything is squared, so both give the reference's W and S_4 -- the S_4 of the two blocks' own
    W would not add up to it"""
    from test_overlap_density import rel_err, s4_of
    from transport_analysis_amd import FourPointStructureFactor
    from transport_analysis_amd._mini_mda import ArrayUniverse

    case = ref.case(100, 1501, 3)
    x, k, lags, W = case[:4]
    u = ArrayUniverse(positions=x.astype(np.float32))
    ok = (100 - lags) >= 2
    s4, unc = s4_of(W, lags, 1501)
    for kw in ({}, {"devices": [0, 0]}):
        r = FourPointStructureFactor(u.atoms, k, lags, cutoff=ref.CUTOFFS, **kw).run().results
        ref.assert_w(r.w_by_origin, case, what=f"class {kw}", extra_bar=1501 * ref.U_R if kw else 0.0)
        err_s, err_u = rel_err(r.s4_by_kvector[:, :, ok], s4[:, :, ok]), rel_err(r.s4_uncentred_by_kvector, unc)
        print(f"    class {kw}: s4 {err_s:.2e}, uncentred {err_u:.2e} relative")
        assert err_s <= 1e-12 and err_u <= 1e-12 and np.all(np.isnan(r.s4_by_kvector[:, :, ~ok]))
    halves = [s4_of(ref.reference(x[:, lo:hi], k, lags, ref.CUTOFFS)[0], lags, 1501)[0] for lo, hi in ((0, 750), (750, 1501))]
    assert float(np.max(np.abs((halves[0] + halves[1])[-1][:, ok] - s4[-1][:, ok]))) > 1e-3  # (k = 0: what summing variances would give)


def test_refuses_2_pow_31_columns():
    """n_atoms dim >= 2^31: TA_E_INVALID before anything is allocated or written.  The slab is device-only, one frame of
    2^30 atoms x 2 float32 columns (never filled).  "fail_alloc_after" 1 makes the call's first workspace request fail with
    TA_E_NOMEM: the refusal comes first, so no workspace was asked for."""
    import torch

    c = _lib.Context(0)
    try:
        c.set_option("stage_device_f32", 1)
        c.stage_alloc_device(1, 2 ** 30, 2, n_slabs=1)
        w = torch.full((1, 1, 1, 1, 2), -7.5, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        c.set_option("fail_alloc_after", 1)
        with pytest.raises(_lib.TAError, match="overlap_density: n_atoms \\* dim must be below 2\\^31") as e:
            c.overlap_density_staged(np.array([[1.0, 0.5]]), [0], 0.5, w.data_ptr())
        assert e.value.code == -1
        c.set_option("fail_alloc_after", 0)
        torch.cuda.synchronize()
        assert bool((w == -7.5).all())
    finally:
        c.close()
