"""k_shell_msd at shapes that reach every branch, through the C-ABI (ta_shell_msd_staged, ta_shell_msd), GPU only.  Every case
runs on a float64 AND a float32 device slab holding the same values, under both conditions, and asserts: sums, count, runs and
nb EQUAL to shell_msd_ref's exact integers AND to the CPU backend's; repeat runs bit-equal; the host-facing entry bit-equal to
the staged one; the staged slab's bits (padding included) unchanged; k_shell_bits, k_shell_msd and k_shell_fold in the kernel
timeline and no widening kernel.

  lags      L = 0, 1, 15, 16, 17, 31, 32, 63, 64, 65, 129 = T - 1 at T = 130; 255, 256, 257 at T = 300 (a workgroup's pass is
            256 lags: 256 is the first lag of the second pass); 1024 at T = 1100.
  frames    T = 1, 2, 63, 64, 65, 128, 129 with L = min(T - 1, 40); T = 1023, 1024, 1025, 2049 with L = 100 and N_b = 5: walks,
            and bond_ref.constructed_levels patterns with runs across the 63|64 and 1023|1024 edges; "shell_msd_chunk" 64
            makes every word edge a chunk edge.
  items     N_b = 1, 2, 3, 63, 64, 65, 1025 at D = 3 and D = 1 (the phantom column, an odd first column, the second b-tile),
            N_a = 1 and 257; T = 65, L = 20.
  boxes     D = 1, 2, 3 with no box, a constant box and per-frame boxes.
  blocks    "pair_chunk" 2 and 5 against automatic, with the launch counts of k_shell_msd.
  A small call straight after a larger one without ta_trim; one case of uniform random float64 positions against a float64
  NumPy evaluation of the definition, within 1e-10 max |S|: the project's stated bound for every path."""
import functools

import numpy as np
import pytest

import bond_ref
import shell_msd_ref as mref
import shell_ref as ref
from test_pair_lifetime import cpu_context
from test_vanhove_distinct_shapes import SLABS, slab_bits, stage, staged_bits
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu


def timeline(c):
    return [n for n, _ in c.kernel_timeline(65536)]


def run_msd(c, dtype, x, condition, L, want, repeat=2, cpu=True, **kw):
    """ta_shell_msd_staged into a caller's device buffers, `repeat` times, and ta_shell_msd: all bit-equal; against want =
    (S, N, runs, nb) of shell_msd_ref and against the CPU backend on the same staged values: for equality"""
    import torch

    T, D = x.shape[0], x.shape[2]
    runs = []
    for _ in range(repeat):
        d_sums = torch.full((L + 1, D), -7.0, dtype=torch.float64, device="cuda:0")
        d_count = torch.full((L + 1,), -7, dtype=torch.int64, device="cuda:0")
        d_runs = torch.full((T + 1,), -7, dtype=torch.int64, device="cuda:0")
        d_nb = torch.full((T,), -7.0, dtype=torch.float64, device="cuda:0")
        c.shell_msd_staged(condition, L, d_sums=d_sums.data_ptr(), d_count=d_count.data_ptr(), d_runs=d_runs.data_ptr(),
                           d_nb=d_nb.data_ptr(), **kw)
        torch.cuda.synchronize()
        runs.append(tuple(v.cpu().numpy() for v in (d_sums, d_count, d_runs, d_nb)))
        names = timeline(c)
        assert {"k_vhd_gather", "k_shell_series", "k_pair_runs", "k_shell_bits", "k_shell_msd", "k_shell_fold"} <= set(names), names
        assert not {"k_pair_series", "k_bond_series", "k_pair_find", "k_widen_f32"} & set(names), names
    for r in runs[1:]:
        assert all(np.array_equal(p, q) for p, q in zip(runs[0], r)), "repeat runs differ"
    host = c.shell_msd(condition, L, **kw)
    assert all(np.array_equal(p, q) for p, q in zip(runs[0], host)), "the host-facing entry differs from the staged one"
    if want is not None:
        for name, got, w in zip(("sums", "count", "runs", "nb"), runs[0], want):
            assert np.array_equal(got, w), (name, condition, np.argwhere(got != w)[:5].tolist())
    if cpu:
        h = cpu_context(x, dtype)
        try:
            twin = h.shell_msd(condition, L, **kw)
        finally:
            h.close()
        assert all(np.array_equal(p, q) for p, q in zip(runs[0], twin)), "the CPU backend differs"
    assert np.array_equal(slab_bits(c, dtype), staged_bits(c, x, dtype)), "the staged slab's bits changed"
    return runs[0]


def run_case(dtype, T, Na, Nb, D, kind, boxed, gap, L, c=None, repeat=2, cpu=True, options=()):
    x, a, b, dims, axes, cuts, g, want, runs, nb = mref.case(T, Na, Nb, D, kind, boxed, gap, L)
    own = c is None
    c = stage(_lib.Context(0) if own else c, x, dtype)
    try:
        for key, value in options:
            c.set_option(key, value)
        for condition in mref.CONDITIONS:
            run_msd(c, dtype, x, condition, L, want[condition] + (runs, nb), repeat=repeat, cpu=cpu, gap=gap, idx_a=a, idx_b=b,
                    dimensions=dims, axes=axes, **cuts)
    finally:
        if own:
            c.close()
    return want


# ---- lags ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SLABS)
def test_lag_counts(dtype):
    """the edges of 16-lag blocks, of a wave and of T - 1 at T = 130, on ONE context"""
    c = _lib.Context(0)
    try:
        for L in (0, 1, 15, 16, 17, 31, 32, 63, 64, 65, 129):
            want = run_case(dtype, 130, 3, 9, 3, "disjoint", True, 1, L, c=c, repeat=1, cpu=L in (0, 65, 129))
        assert want["continuous"][1][0] > 0
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T,L", [(300, 255), (300, 256), (300, 257), (1100, 1024)])
def test_lags_beyond_one_pass(T, L, dtype):
    """a workgroup's pass holds 256 lags: 255 fills it, 256 is the first lag of the second pass; all-inside items among the
    walkers make the long lags count"""
    x, a, b, dims, axes, cuts, s, _ = ref.case(T, 2, 4, 3, "disjoint", False, 0)
    x = np.array(x)
    x[:, b[0]] = x[:, a[0]] + 0.125  # (one observed item rides along with a reference item: inside in every frame)
    g = ref.filtered(ref.levels(x, a, b, None, **cuts), 0)
    assert g[0].all()
    c = stage(_lib.Context(0), x, dtype)
    try:
        for condition in mref.CONDITIONS:
            S, N = mref.gated_sums(x, b, g, L, condition)
            runs, nb = mref.check_counts(g, L, N, condition)
            assert N[L] >= T - L
            run_msd(c, dtype, x, condition, L, (S, N, runs, nb), repeat=1, idx_a=a, idx_b=b, **cuts)
    finally:
        c.close()


# ---- frame counts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 128, 129, 1023, 1024, 1025, 2049])
def test_frame_counts_walk(T, dtype):
    L = min(T - 1, 40) if T < 1000 else 100
    run_case(dtype, T, 3, 5, 3, "disjoint", "frames", 2, L, repeat=1)
    run_case(dtype, T, 3, 5, 3, "disjoint", "frames", 2, L, repeat=1, cpu=False, options=(("shell_msd_chunk", 64),))


@functools.lru_cache(maxsize=None)
def pattern_case(T, gap, L):
    """bond_ref.constructed_levels(T, gap) around three reference items, the owner changing every 7 frames, every observed item
    moving by a few grid steps per frame along the third axis (at most 48 steps away: far inside the margins between
    shell_ref.LEVEL_DISTANCE and the cutoffs, and the levels are asserted): (x, a, b, {condition: (S, N, runs, nb)})"""
    lv = bond_ref.constructed_levels(T, gap)
    owner = (np.arange(lv.shape[0])[:, None] + np.arange(T)[None, :] // 7) % 3
    x, a, b = ref.pattern_positions(lv, owner, n_ref=3)
    x = np.array(x)
    x[:, b, 2] = (np.arange(T)[:, None] % 17) / 1024.0 * (1 + np.arange(b.size)[None, :] % 3)
    assert np.array_equal(ref.levels(x, a, b, None, **ref.PATTERN_CUTS), lv)
    g = ref.filtered(lv, gap)
    want = {}
    for condition in mref.CONDITIONS:
        S, N = mref.gated_sums(x, b, g, L, condition)
        want[condition] = (S, N) + mref.check_counts(g, L, N, condition)
    x.setflags(write=False)
    return x, a, b, want


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T", [63, 64, 65, 129, 1023, 1024, 1025])
def test_frame_counts_patterns(T, dtype):
    """runs and absences across the 63|64 and 1023|1024 edges, with the default chunk and with every word edge a chunk edge"""
    L = min(T - 1, 100)
    c = _lib.Context(0)
    try:
        for gap, chunk in ((0, 0), (1, 64), (63, 128)):
            x, a, b, want = pattern_case(T, gap, L)
            stage(c, x, dtype)
            c.set_option("shell_msd_chunk", chunk)
            for condition in mref.CONDITIONS:
                run_msd(c, dtype, x, condition, L, want[condition], repeat=1, cpu=gap == 1, gap=gap, idx_a=a, idx_b=b, **ref.PATTERN_CUTS)
    finally:
        c.close()


# ---- item counts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("D", [3, 1])
@pytest.mark.parametrize("Nb", [1, 2, 3, 63, 64, 65, 1025])
def test_observed_item_counts(Nb, D, dtype):
    run_case(dtype, 65, 3, Nb, D, "disjoint", True, 1, 20, repeat=1)


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("Na", [1, 257])
def test_reference_item_counts(Na, dtype):
    run_case(dtype, 65, Na, 65, 3, "disjoint", True, 1, 20, repeat=1)


# ---- dimensions and boxes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("D", [1, 2, 3])
def test_dimensions_and_boxes(D, dtype):
    for boxed in (False, True, "frames"):
        want = run_case(dtype, 70, 7, 131, D, "disjoint", boxed, 2, 30)
        assert want["continuous"][1][10] > 0 and want["endpoints"][1][30] > want["continuous"][1][30]  # (the conditions differ)
    run_case(dtype, 70, 0, 131, D, "same", True, 0, 30, repeat=1)


# ---- blocks of observed items ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SLABS)
def test_blocks_bit_equal(dtype):
    """15 pattern rows at T = 300: "pair_chunk" 2 and 5 (blocks of 4: a block starts at an even item) against automatic"""
    gap, L = 2, 120
    x, a, b, want = pattern_case(300, gap, L)
    N = b.size
    c = stage(_lib.Context(0), x, dtype)
    try:
        for condition in mref.CONDITIONS:
            got = []
            for items, blocks in ((0, 1), (2, (N + 1) // 2), (5, (N + 3) // 4), (1000, 1)):
                c.set_option("pair_chunk", items)
                got.append(run_msd(c, dtype, x, condition, L, want[condition], repeat=1, cpu=False, gap=gap, idx_a=a, idx_b=b,
                                   **ref.PATTERN_CUTS))
                for name in ("k_shell_msd", "k_shell_bits", "k_shell_fold", "k_pair_filter"):
                    assert c.kernel_launches(name) == blocks, (name, items)
            for r in got[1:]:
                assert all(np.array_equal(p, q) for p, q in zip(got[0], r))
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_stale_state(dtype):
    """a small call, a larger one, then small ones again on ONE context without ta_trim: the words, the partial rows and the
    level block of the larger call are still there"""
    c = _lib.Context(0)
    try:
        for T, Na, Nb, L in ((7, 2, 3, 6), (131, 9, 1030, 130), (7, 2, 3, 3), (65, 2, 2, 10)):
            run_case(dtype, T, Na, Nb, 3, "disjoint", True, 1, L, c=c, repeat=1, cpu=False)
    finally:
        c.close()


def test_outputs_one_at_a_time():
    """every output alone, the others NULL: the same bits as all four at once"""
    import torch

    x, a, b, dims, axes, cuts, g, want, runs, nb = mref.case(70, 7, 45, 3, "disjoint", True, 1, 30)
    c = stage(_lib.Context(0), x, np.float64)
    try:
        kw = dict(gap=1, idx_a=a, idx_b=b, dimensions=dims, axes=axes, **cuts)
        full = want["endpoints"] + (runs, nb)
        for i, key in enumerate(("sums", "count", "runs", "nb")):
            only = c.shell_msd("endpoints", 30, **{k: k == key for k in ("sums", "count", "runs", "nb")}, **kw)
            assert [v is not None for v in only] == [j == i for j in range(4)] and np.array_equal(only[i], full[i])
        d_count = torch.full((31,), -7, dtype=torch.int64, device="cuda:0")
        c.shell_msd_staged("continuous", 30, d_count=d_count.data_ptr(), **kw)
        torch.cuda.synchronize()
        assert np.array_equal(d_count.cpu().numpy(), want["continuous"][1])
    finally:
        c.close()


def test_non_grid_input_within_the_bound():
    """uniform random float64 positions (not on any grid), float64 slab: sums within 1e-10 max |S| of a float64 NumPy evaluation
    of the definition; counts, runs, nb equal to the CPU backend's"""
    rng = np.random.default_rng(5)
    T, A, L = 200, 40, 150
    x = np.cumsum(rng.normal(scale=0.05, size=(T, A, 3)), axis=0) + rng.uniform(0.0, 2.0, size=(1, A, 3))
    a, b = np.arange(8), np.arange(8, A)
    c = stage(_lib.Context(0), x, np.float64)
    h = cpu_context(x, np.float64)
    try:
        for condition in mref.CONDITIONS:
            kw = dict(r_cut=0.6, r_break=0.75, gap=1, idx_a=a, idx_b=b)
            S, N, runs, nb = c.shell_msd(condition, L, **kw)
            assert np.array_equal(S, c.shell_msd(condition, L, **kw)[0]), "repeat runs differ"
            twin = h.shell_msd(condition, L, **kw)
            assert np.array_equal(N, twin[1]) and np.array_equal(runs, twin[2]) and np.array_equal(nb, twin[3])
            # g from nb is not per item: take it from one-item calls of the CPU backend
            g = np.stack([h.shell_msd(condition, 0, sums=False, count=False, runs=False, **{**kw, "idx_b": b[q:q + 1]})[3] for q in range(b.size)]) > 0
            want = np.zeros((L + 1, 3))
            xb = x[:, b].transpose(1, 0, 2)
            w = g.copy()
            for tau in range(L + 1):
                if tau:
                    w = (w[:, :-1] & g[:, tau:]) if condition == "continuous" else (g[:, :T - tau] & g[:, tau:])
                d = xb[:, tau:] - xb[:, :T - tau]
                want[tau] = (d * d * w[:, :, None]).sum(axis=(0, 1))
                assert N[tau] == w.sum()
            bound = 1e-10 * np.abs(want).max()
            err = np.abs(S - want).max()
            print(f"    {condition}: max |S - numpy| = {err:.3e}, bound {bound:.3e}; CPU twin {np.abs(twin[0] - want).max():.3e}")
            assert err <= bound and np.abs(twin[0] - want).max() <= bound and N[100] > 0
    finally:
        c.close()
        h.close()


def test_refusals_on_the_device():
    x, a, b, dims, axes, cuts, g, want, runs, nb = mref.case(70, 7, 45, 3, "disjoint", True, 1, 30)
    c = stage(_lib.Context(0), x, np.float64)
    try:
        for L, text in ((-1, "max_lag must be 0 ... n_frames - 1 = 69"), (70, "max_lag must be 0 ... n_frames - 1 = 69")):
            with pytest.raises(_lib.TAError, match=text):
                c.shell_msd("continuous", L, idx_a=a, idx_b=b, **cuts)
        with pytest.raises(_lib.TAError, match="shell_msd_chunk: 0 \\(automatic\\) or the origin frames per staged chunk"):
            c.set_option("shell_msd_chunk", -1)
    finally:
        c.close()
