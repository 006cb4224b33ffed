"""k_shell_orient at shapes that reach every branch, through the C-ABI (ta_shell_orient_staged, ta_shell_orient), GPU only.
Every case runs on a float64 AND a float32 device slab holding the same values, under both conditions, and asserts: sums,
count, runs and nb EQUAL to shell_orient_ref's exact integers AND to the CPU backend's; repeat runs bit-equal; the host-facing
entry bit-equal to the staged one; the staged slab's bits (padding included) unchanged; k_shell_bits, k_shell_orient and
k_shell_fold in the kernel timeline and no k_orient, k_shell_msd or k_widen_f32.

  lags      L = 0, 1, 63, 64, 65, 129 = T - 1 at T = 130; 255, 256, 257 at T = 300 (a workgroup's pass is 256 lags: 256 is the
            first lag of the second pass).
  frames    T = 1, 2, 63, 64, 65, 129, 1025 with L = min(T - 1, 40) (100 at T = 1025), with the default chunk and with
            "shell_msd_chunk" 64, which makes every word edge a chunk edge.
  items     N_b = 1, 2, 3, 65, 1025 (odd counts: the phantom column of Z; the second b-tile), N_a = 1 and 257; T = 65, L = 20.
  modes     bond, bisector, normal with no box, a constant box and per-frame boxes, the anchor in column 0 and 1.
  blocks    "pair_chunk" 2 and 5 against automatic, with the launch counts of k_shell_orient.
  A small call straight after a larger one without ta_trim; one case of uniform random float64 positions with vectors along
  no axis against a float64 NumPy evaluation of the definition, within 1e-10 max |S|: the project's stated bound for every
  path."""
import numpy as np
import pytest

import shell_orient_ref as oref
import shell_ref as ref
from test_pair_lifetime import cpu_context
from test_vanhove_distinct_shapes import SLABS, slab_bits, stage, staged_bits
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu


def timeline(c):
    return [n for n, _ in c.kernel_timeline(65536)]


def run_orient(c, dtype, x, condition, L, rows, mode, want, repeat=2, cpu=True, **kw):
    """ta_shell_orient_staged into a caller's device buffers, `repeat` times, and ta_shell_orient: all bit-equal; against want =
    (S, N, runs, nb) of shell_orient_ref and against the CPU backend on the same staged values: for equality"""
    import torch

    T = x.shape[0]
    runs = []
    for _ in range(repeat):
        d_sums = torch.full((L + 1, 2), -7.0, dtype=torch.float64, device="cuda:0")
        d_count = torch.full((L + 1,), -7, dtype=torch.int64, device="cuda:0")
        d_runs = torch.full((T + 1,), -7, dtype=torch.int64, device="cuda:0")
        d_nb = torch.full((T,), -7.0, dtype=torch.float64, device="cuda:0")
        c.shell_orient_staged(condition, L, rows, mode, d_sums=d_sums.data_ptr(), d_count=d_count.data_ptr(), d_runs=d_runs.data_ptr(),
                              d_nb=d_nb.data_ptr(), **kw)
        torch.cuda.synchronize()
        runs.append(tuple(v.cpu().numpy() for v in (d_sums, d_count, d_runs, d_nb)))
        names = timeline(c)
        assert {"k_vhd_gather", "k_shell_series", "k_pair_runs", "k_shell_bits", "k_shell_orient", "k_shell_fold"} <= set(names), names
        assert not {"k_orient", "k_shell_msd", "k_widen_f32", "k_pair_series", "k_bond_series"} & set(names), names
    for r in runs[1:]:
        assert all(np.array_equal(p, q) for p, q in zip(runs[0], r)), "repeat runs differ"
    host = c.shell_orient(condition, L, rows, mode, **kw)
    assert all(np.array_equal(p, q) for p, q in zip(runs[0], host)), "the host-facing entry differs from the staged one"
    if want is not None:
        for name, got, w in zip(("sums", "count", "runs", "nb"), runs[0], want):
            assert np.array_equal(got, w), (name, condition, np.argwhere(got != w)[:5].tolist())
    if cpu:
        h = cpu_context(x, dtype)
        try:
            twin = h.shell_orient(condition, L, rows, mode, **kw)
        finally:
            h.close()
        assert all(np.array_equal(p, q) for p, q in zip(runs[0], twin)), "the CPU backend differs"
    assert np.array_equal(slab_bits(c, dtype), staged_bits(c, x, dtype)), "the staged slab's bits changed"
    return runs[0]


def run_case(dtype, T, Na, Nb, kind, boxed, gap, L, mode="bisector", anchor=0, c=None, repeat=2, cpu=True, options=()):
    x, a, b, rows, dims, axes, cuts, g, want, runs, nb = oref.case(T, Na, Nb, kind, boxed, gap, L, mode, anchor)
    own = c is None
    c = stage(_lib.Context(0) if own else c, x, dtype)
    try:
        for key, value in options:
            c.set_option(key, value)
        for condition in oref.CONDITIONS:
            run_orient(c, dtype, x, condition, L, rows, mode, want[condition] + (runs, nb), repeat=repeat, cpu=cpu, anchor=anchor, gap=gap,
                       idx_a=a, idx_b=b, dimensions=dims, axes=axes, **cuts)
    finally:
        if own:
            c.close()
    return want


# ---- lags ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SLABS)
def test_lag_counts(dtype):
    """the edges of a wave and of T - 1 at T = 130, on ONE context"""
    c = _lib.Context(0)
    try:
        for L in (0, 1, 63, 64, 65, 129):
            want = run_case(dtype, 130, 3, 9, "disjoint", True, 1, L, c=c, repeat=1, cpu=L in (0, 65, 129))
        assert want["continuous"][1][0] > 0
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("L", [255, 256, 257])
def test_lags_beyond_one_pass(L, dtype):
    """T = 300: 255 fills a workgroup's pass of 256 lags, 256 is the first lag of the second pass; an anchor that rides along
    with a reference item (inside in every frame) makes the long lags count"""
    T = 300
    x, a, b, dims, axes, cuts, s, _ = ref.case(T, 2, 4, 3, "disjoint", False, 0)
    x = np.array(x)
    x[:, b[0]] = x[:, a[0]] + 0.125
    g = ref.filtered(ref.levels(x, a, b, None, **cuts), 0)
    assert g[0].all()
    x2, rows = oref.with_partners(x, b, "normal", 0, None, 5)
    u = oref.unit_vectors(x2, rows, "normal", None)
    c = stage(_lib.Context(0), x2, dtype)
    try:
        for condition in oref.CONDITIONS:
            S, N = oref.gated_sums(u, g, L, condition)
            runs, nb = oref.mref.check_counts(g, L, N, condition)
            assert N[L] >= T - L and S[L, 1] > 0
            run_orient(c, dtype, x2, condition, L, rows, "normal", (S, N, runs, nb), repeat=1, idx_a=a, idx_b=b, **cuts)
    finally:
        c.close()


# ---- frame counts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 129, 1025])
def test_frame_counts(T, dtype):
    L = min(T - 1, 40) if T < 1000 else 100
    run_case(dtype, T, 3, 5, "disjoint", "frames", 2, L, repeat=1)
    run_case(dtype, T, 3, 5, "disjoint", "frames", 2, L, repeat=1, cpu=False, options=(("shell_msd_chunk", 64),))


# ---- item counts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("Nb", [1, 2, 3, 65, 1025])
def test_observed_item_counts(Nb, dtype):
    run_case(dtype, 65, 3, Nb, "disjoint", True, 1, 20, repeat=1)


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("Na", [1, 257])
def test_reference_item_counts(Na, dtype):
    run_case(dtype, 65, Na, 65, "disjoint", True, 1, 20, repeat=1)


# ---- modes and boxes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("mode", oref.MODES)
def test_modes_and_boxes(mode, dtype):
    for boxed, anchor in ((False, 0), (True, 1), ("frames", 0)):
        want = run_case(dtype, 70, 7, 131, "disjoint", boxed, 2, 30, mode=mode, anchor=anchor)
        assert want["continuous"][1][10] > 0 and want["endpoints"][1][30] > want["continuous"][1][30]  # (the conditions differ)
    run_case(dtype, 70, 0, 131, "same", True, 0, 30, mode=mode, anchor=1, repeat=1)


# ---- blocks of observed items ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SLABS)
def test_blocks_bit_equal(dtype):
    """15 anchors at T = 130: "pair_chunk" 2 and 5 (blocks of 4: a block starts at an even item) against automatic"""
    gap, L, N = 2, 100, 15
    x, a, b, rows, dims, axes, cuts, g, want, runs, nb = oref.case(130, 3, N, "disjoint", "frames", gap, L, "bisector", 1)
    c = stage(_lib.Context(0), x, dtype)
    try:
        for condition in oref.CONDITIONS:
            got = []
            for items, blocks in ((0, 1), (2, (N + 1) // 2), (5, (N + 3) // 4), (1000, 1)):
                c.set_option("pair_chunk", items)
                got.append(run_orient(c, dtype, x, condition, L, rows, "bisector", want[condition] + (runs, nb), repeat=1, cpu=False, anchor=1,
                                      gap=gap, idx_a=a, idx_b=b, dimensions=dims, axes=axes, **cuts))
                for name in ("k_shell_orient", "k_shell_bits", "k_shell_fold", "k_pair_filter"):
                    assert c.kernel_launches(name) == blocks, (name, items)
            for r in got[1:]:
                assert all(np.array_equal(p, q) for p, q in zip(got[0], r))
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_stale_state(dtype):
    """a small call, a larger one, then small ones again on ONE context without ta_trim: the words, the partial rows, the index
    rows and the level block of the larger call are still there"""
    c = _lib.Context(0)
    try:
        for T, Na, Nb, L, mode in ((7, 2, 3, 6, "bond"), (131, 9, 1030, 130, "normal"), (7, 2, 3, 3, "bisector"), (65, 2, 2, 10, "bond")):
            run_case(dtype, T, Na, Nb, "disjoint", True, 1, L, mode=mode, c=c, repeat=1, cpu=False)
    finally:
        c.close()


def test_non_grid_input_within_the_bound():
    """uniform random float64 positions (not on any grid; vectors along no axis, some through a face of the box), float64 slab:
    sums within 1e-10 max |S| of a float64 NumPy evaluation of the definition; counts, runs, nb equal to the CPU backend's"""
    rng = np.random.default_rng(5)
    T, n_ref, nv, L = 200, 8, 32, 150
    box = np.array([4.0, 4.0, 4.0])
    dims = np.tile([4.0, 4.0, 4.0, 90.0, 90.0, 90.0], (T, 1))
    centre = np.cumsum(rng.normal(scale=0.05, size=(T, n_ref + nv, 3)), axis=0) + rng.uniform(0.0, 2.0, size=(1, n_ref + nv, 3))
    centre[:, n_ref] = centre[:, 0] + np.array([0.1, 0.05, 0.02])  # (one anchor rides along with a reference item: long runs)
    arms = []
    for _ in range(2):  # two arms per anchor that turn slowly
        w = np.cumsum(rng.normal(scale=0.15, size=(T, nv, 3)), axis=0) + rng.normal(size=(1, nv, 3))
        arm = 0.3 * w / np.linalg.norm(w, axis=2, keepdims=True)
        arms.append(centre[:, n_ref:] + arm + rng.integers(-1, 2, size=(T, nv, 3)) * box)
    x = np.concatenate([centre] + arms, axis=1)
    a, b = np.arange(n_ref), np.arange(n_ref, n_ref + nv)
    c = stage(_lib.Context(0), x, np.float64)
    h = cpu_context(x, np.float64)
    try:
        kw = dict(r_cut=0.6, r_break=0.75, gap=1, idx_a=a, idx_b=b, dimensions=dims, axes=(0, 1, 2))
        # g per item: from one-item calls of the CPU backend's residence series
        g = np.stack([h.shell_residence(0, 0.6, r_break=0.75, gap=1, idx_a=a, idx_b=b[q:q + 1], dimensions=dims, axes=(0, 1, 2),
                                        ci=False, runs=False)[2] for q in range(nv)]) > 0
        for mode in oref.MODES:
            K = oref.ROW_LEN[mode]
            rows = np.stack([b] + [n_ref + nv * (1 + j) + np.arange(nv) for j in range(K - 1)], axis=1).astype(np.int32)
            for condition in oref.CONDITIONS:
                S, N, runs, nb = c.shell_orient(condition, L, rows, mode, **kw)
                assert np.array_equal(S, c.shell_orient(condition, L, rows, mode, **kw)[0]), "repeat runs differ"
                twin = h.shell_orient(condition, L, rows, mode, **kw)
                assert np.array_equal(N, twin[1]) and np.array_equal(runs, twin[2]) and np.array_equal(nb, twin[3])
                want, n_want = oref.float_sums(x, rows, mode, box, g, L, condition)
                assert np.array_equal(N, n_want)
                bound = 1e-10 * np.abs(want).max()
                err = np.abs(S - want).max()
                print(f"    {mode} {condition}: max |S - numpy| = {err:.3e}, bound {bound:.3e}; CPU twin {np.abs(twin[0] - want).max():.3e}")
                assert err <= bound and np.abs(twin[0] - want).max() <= bound and N[100] > 0
    finally:
        c.close()
        h.close()


def test_outputs_one_at_a_time_and_refusals_on_the_device():
    import torch

    x, a, b, rows, dims, axes, cuts, g, want, runs, nb = oref.case(70, 7, 45, "disjoint", True, 1, 30, "bond")
    c = stage(_lib.Context(0), x, np.float64)
    try:
        kw = dict(gap=1, idx_a=a, idx_b=b, dimensions=dims, axes=axes, **cuts)
        full = want["endpoints"] + (runs, nb)
        for i, key in enumerate(("sums", "count", "runs", "nb")):
            only = c.shell_orient("endpoints", 30, rows, "bond", **{k: k == key for k in ("sums", "count", "runs", "nb")}, **kw)
            assert [v is not None for v in only] == [j == i for j in range(4)] and np.array_equal(only[i], full[i])
        d_count = torch.full((31,), -7, dtype=torch.int64, device="cuda:0")
        c.shell_orient_staged("continuous", 30, rows, "bond", d_count=d_count.data_ptr(), **kw)
        torch.cuda.synchronize()
        assert np.array_equal(d_count.cpu().numpy(), want["continuous"][1])
        for L, text in ((-1, "max_lag must be 0 ... n_frames - 1 = 69"), (70, "max_lag must be 0 ... n_frames - 1 = 69")):
            with pytest.raises(_lib.TAError, match=text):
                c.shell_orient("continuous", L, rows, "bond", **kw)
        with pytest.raises(_lib.TAError, match="shell_orient: the anchor of vector 0"):
            c.shell_orient("continuous", 30, rows, "bond", anchor=1, **kw)
    finally:
        c.close()
