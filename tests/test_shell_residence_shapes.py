"""k_shell_series at shapes that reach every branch, through the C-ABI (ta_shell_residence_staged, ta_shell_residence), GPU
only.  Every case runs on a float64 AND a float32 device slab holding the same values and asserts k_vhd_gather and
k_shell_series in the kernel timeline, k_pair_filter there exactly when the call needs it, that no pair-resolved series
kernel and no widening kernel ran, the run lengths, inside counts and (fft = 0) lag sums EQUAL to shell_ref's AND to the CPU
backend's, repeat runs bit-equal, the staged slab's bits (padding included) unchanged, and the host-facing entry bit-equal to
the staged one with device outputs.

  items     N_b = 1, 2, 3, 63, 64, 65, 127, 1023, 1024, 1025, 2049 (the phantom column, word edges, b-tile edges) and
            N_a = 1, 2, 255, 256, 257, 513, on walks of 65 frames in a box.
  frames    T = 1, 2, 63, 64, 65, 128, 129, 1023, 1024, 1025, 2049 (partial words, the zero rows up to the pitch, the second
            1024-frame row of the block): a walk, and bond_ref.constructed_levels realised around three reference items with
            the owner changing every 7 frames: runs and absences across the 63|64 and 1023|1024 edges.
  boxes     D = 1, 2, 3 with no box, a constant box and per-frame boxes; the same list.
  chunks    "shell_chunk" 1 and 3 and "pair_chunk" 2 and 5 against the automatic values, with the launch counts: with
            "shell_chunk" 1 every word edge is a chunk edge.
  A small call straight after a larger one without ta_trim (stale scratch, a stale level block); fft = 1 within 1e-10 of ci[0]."""
import functools

import numpy as np
import pytest

import bond_ref
import shell_ref as ref
from test_pair_lifetime import cpu_context
from test_vanhove_distinct_shapes import SLABS, slab_bits, stage, staged_bits
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu


def timeline(c):
    return [n for n, _ in c.kernel_timeline(65536)]


def run_shell(c, dtype, x, fft, want, filtered, repeat=2, cpu=True, **kw):
    """ta_shell_residence_staged into a caller's device buffers, `repeat` times, and ta_shell_residence: all bit-equal; against
    want = (ci, runs, nb, ...) of shell_ref (None: not compared) and against the CPU backend on the same staged values"""
    import torch

    T = x.shape[0]
    runs = []
    for _ in range(repeat):
        d_ci = torch.full((T,), -7.0, dtype=torch.float64, device="cuda:0")
        d_runs = torch.full((T + 1,), -7, dtype=torch.int64, device="cuda:0")
        d_nb = torch.full((T,), -7.0, dtype=torch.float64, device="cuda:0")
        c.shell_residence_staged(fft, d_ci=d_ci.data_ptr(), d_runs=d_runs.data_ptr(), d_nb=d_nb.data_ptr(), **kw)
        torch.cuda.synchronize()
        runs.append((d_ci.cpu().numpy(), d_runs.cpu().numpy(), d_nb.cpu().numpy()))
        names = timeline(c)
        assert "k_vhd_gather" in names and "k_shell_series" in names and "k_pair_runs" in names and "k_pair_reduce" in names, names
        assert ("k_pair_filter" in names) == filtered, (filtered, names)
        assert not {"k_pair_series", "k_bond_series", "k_pair_find", "k_widen_f32"} & set(names), names
    for r in runs[1:]:
        assert all(np.array_equal(p, q) for p, q in zip(runs[0], r)), "repeat runs differ"
    host = c.shell_residence(fft, **kw)
    assert all(np.array_equal(p, q) for p, q in zip(runs[0], host)), "the host-facing entry differs from the staged one"
    ci, rl, nb = runs[0]
    if want is not None:
        assert np.array_equal(rl, want[1]), np.flatnonzero(rl != want[1])[:5]
        assert np.array_equal(nb, want[2]), np.flatnonzero(nb != want[2])[:5]
        if fft:
            err = float(np.max(np.abs(ci - want[0])))
            print(f"    fft: max |ci - exact| = {err:.3e}, bound {1e-10 * max(float(want[0][0]), 1.0):.3e}")
            assert err <= 1e-10 * max(float(want[0][0]), 1.0)
        else:
            assert np.array_equal(ci, want[0]), np.flatnonzero(ci != want[0])[:5]
    if cpu and not fft:
        h = cpu_context(x, dtype)
        try:
            w_ci, w_runs, w_nb = h.shell_residence(0, **kw)
        finally:
            h.close()
        assert np.array_equal(rl, w_runs) and np.array_equal(nb, w_nb) and np.array_equal(ci, w_ci), "the CPU backend differs"
    assert np.array_equal(slab_bits(c, dtype), staged_bits(c, x, dtype)), "the staged slab's bits changed"
    return runs[0]


def run_case(dtype, T, Na, Nb, D, kind, boxed, gap, ffts=(0,), c=None):
    x, a, b, dims, axes, cuts, s, want = ref.case(T, Na, Nb, D, kind, boxed, gap)
    own = c is None
    c = stage(_lib.Context(0) if own else c, x, dtype)
    try:
        for fft in ffts:
            run_shell(c, dtype, x, fft, want, True, repeat=2 if fft == 0 else 1, gap=gap, idx_a=a, idx_b=b, dimensions=dims, axes=axes, **cuts)
    finally:
        if own:
            c.close()
    return s, want


# ---- item counts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("Nb", [1, 2, 3, 63, 64, 65, 127, 1023, 1024, 1025, 2049])
def test_observed_item_counts(Nb, dtype):
    s, want = run_case(dtype, 65, 3, Nb, 3, "disjoint", True, 1)
    if Nb >= 63:
        assert 0 < want[2].sum() < s.size


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("Na", [1, 2, 255, 256, 257, 513])
def test_reference_item_counts(Na, dtype):
    s, want = run_case(dtype, 65, Na, 65, 3, "disjoint", True, 1)
    assert 0 < want[2].sum() < s.size


@pytest.mark.parametrize("dtype", SLABS)
def test_both_tiles_crossed(dtype):
    """257 reference items (the walk's second 256) against 1025 observed items (the second b-tile), 3 frames; the same list of
    1025 items (self excluded on both sides of the tile edge)"""
    run_case(dtype, 3, 257, 1025, 3, "disjoint", "frames", 0)
    run_case(dtype, 3, 0, 1025, 2, "same", True, 0)


# ---- frame counts -------------------------------------------------------------------------------------------------------------
TS = [1, 2, 63, 64, 65, 128, 129, 1023, 1024, 1025, 2049]


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T", TS)
def test_frame_counts_walk(T, dtype):
    run_case(dtype, T, 3, 5, 3, "disjoint", "frames", 2, ffts=(0, 1))


@functools.lru_cache(maxsize=None)
def pattern_case(T, gap):
    """bond_ref.constructed_levels(T, gap) around three reference items, the owner changing every 7 frames: (x, a, b, sums)"""
    lv = bond_ref.constructed_levels(T, gap)
    owner = (np.arange(lv.shape[0])[:, None] + np.arange(T)[None, :] // 7) % 3
    x, a, b = ref.pattern_positions(lv, owner, n_ref=3)
    assert np.array_equal(ref.levels(x, a, b, None, **ref.PATTERN_CUTS), lv)
    x.setflags(write=False)
    return x, a, b, ref.sums(ref.filtered(lv, gap))


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T", TS)
def test_frame_counts_patterns(T, dtype):
    c = _lib.Context(0)
    try:
        for gap in (0, 1, 63):
            x, a, b, want = pattern_case(T, gap)
            stage(c, x, dtype)
            run_shell(c, dtype, x, 0, want, True, repeat=1, gap=gap, idx_a=a, idx_b=b, **ref.PATTERN_CUTS)
    finally:
        c.close()


# ---- dimensions and boxes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("D", [1, 2, 3])
def test_dimensions_and_boxes(D, dtype):
    """walks of 70 frames, 7 reference and 131 observed items (the phantom column): no box, the constant box, per-frame boxes;
    D = 2 on the box axes {0, 2}, D = 1 on axis 1; the same list in the constant box"""
    seen = set()
    for boxed in (False, True, "frames"):
        s, want = run_case(dtype, 70, 7, 131, D, "disjoint", boxed, 2, ffts=(0, 1))
        assert 0 < want[2].sum() < s.size
        seen |= set(np.unique(s).tolist())
    assert seen == {0, 1, 2}
    run_case(dtype, 70, 0, 131, D, "same", True, 0)


@pytest.mark.parametrize("dtype", SLABS)
def test_filter_runs_exactly_when_needed(dtype):
    """gap = 0 and r_break = r_cut: no k_pair_filter launch, level 2 is written as 1.0; the series is then form itself"""
    x, a, b, dims, axes, cuts, s, _ = ref.case(70, 7, 131, 3, "disjoint", True, 0)
    c = stage(_lib.Context(0), x, dtype)
    try:
        box = dict(idx_a=a, idx_b=b, dimensions=dims, axes=axes)
        run_shell(c, dtype, x, 0, ref.sums(s == 2), False, r_cut=cuts["r_cut"], **box)
        run_shell(c, dtype, x, 0, ref.sums(s >= 1), False, repeat=1, r_cut=cuts["r_break"], r_break=cuts["r_break"], **box)
        run_shell(c, dtype, x, 0, ref.sums(ref.filtered(s, 0)), True, repeat=1, **cuts, **box)
        run_shell(c, dtype, x, 0, ref.sums(ref.filtered(np.where(s == 2, 2, 0), 3)), True, repeat=1, r_cut=cuts["r_cut"], gap=3, **box)
    finally:
        c.close()


# ---- the two chunkings --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", SLABS)
def test_chunks_bit_equal(dtype):
    """T = 300 (5 words), 15 pattern rows whose runs and absences cross word edges: "shell_chunk" 1 (every word edge a chunk
    edge), 3 and automatic; "pair_chunk" 2, 5 (blocks of 4: a block starts at an even item) and automatic; both at once"""
    gap = 2
    x, a, b, want = pattern_case(300, gap)
    N = b.size
    c = stage(_lib.Context(0), x, dtype)
    try:
        runs = []
        by2, by4 = (N + 1) // 2, (N + 3) // 4
        for words, items, passes, blocks in ((0, 0, 1, 1), (1, 0, 5, 1), (3, 0, 2, 1), (0, 2, 1, by2), (0, 5, 1, by4), (1, 2, 5, by2),
                                             (1000, 1000, 1, 1)):
            c.set_option("shell_chunk", words)
            c.set_option("pair_chunk", items)
            runs.append(run_shell(c, dtype, x, 0, want, True, repeat=1, gap=gap, idx_a=a, idx_b=b, **ref.PATTERN_CUTS))
            # (the counters are the last call's)
            assert c.kernel_launches("k_shell_series") == passes * blocks == c.kernel_launches("k_vhd_gather"), (words, items)
            assert c.kernel_launches("k_pair_filter") == blocks == c.kernel_launches("k_pair_runs"), (words, items)
        for r in runs[1:]:
            assert all(np.array_equal(p, q) for p, q in zip(runs[0], r))
        c.set_option("shell_chunk", 2)
        c.set_option("pair_chunk", 5)
        run_shell(c, dtype, x, 1, want, True, repeat=1, gap=gap, idx_a=a, idx_b=b, **ref.PATTERN_CUTS)
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_chunks_on_a_walk_with_two_tiles(dtype):
    """1025 observed items in blocks of 600 (the second block starts inside the first b-tile and ends in the second) and
    words one at a time, 130 frames in per-frame boxes, against the automatic values"""
    x, a, b, dims, axes, cuts, s, want = ref.case(130, 5, 1025, 3, "disjoint", "frames", 1)
    c = stage(_lib.Context(0), x, dtype)
    try:
        kw = dict(gap=1, idx_a=a, idx_b=b, dimensions=dims, axes=axes, **cuts)
        base = run_shell(c, dtype, x, 0, want, True, repeat=1, **kw)
        c.set_option("shell_chunk", 1)
        c.set_option("pair_chunk", 601)
        got = run_shell(c, dtype, x, 0, want, True, repeat=1, cpu=False, **kw)
        assert c.kernel_launches("k_shell_series") == 3 * 2
        assert all(np.array_equal(p, q) for p, q in zip(base, got))
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_stale_scratch(dtype):
    """a small call, a larger one, then the small one again on ONE context without ta_trim: the gathered scratch and the level
    block of the larger call are still there"""
    c = _lib.Context(0)
    try:
        for T, Na, Nb in ((7, 2, 3), (131, 9, 1030), (7, 2, 3), (65, 2, 2)):
            run_case(dtype, T, Na, Nb, 3, "disjoint", True, 1, c=c)
    finally:
        c.close()


def test_refuses_2_pow_31_columns():
    """n_atoms dim >= 2^31: TA_E_INVALID before anything is allocated or written"""
    import torch

    c = _lib.Context(0)
    try:
        c.set_option("stage_device_f32", 1)
        c.stage_alloc_device(1, 2 ** 30, 2)
        out = torch.full((2,), -7, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        c.set_option("fail_alloc_after", 1)
        with pytest.raises(_lib.TAError, match="shell_residence: n_atoms \\* dim must be below 2\\^31") as e:
            c.shell_residence_staged(0, 0.5, idx_a=[0], idx_b=[1], d_runs=out.data_ptr())
        assert e.value.code == -1
        c.set_option("fail_alloc_after", 0)
        torch.cuda.synchronize()
        assert bool((out == -7).all())
    finally:
        c.close()
