"""k_pair_find, k_pair_count, k_pair_list, k_pair_series and k_pair_runs at shapes that reach every branch, through the C-ABI
(ta_pair_find, ta_pair_find_read, ta_pair_lifetime_staged, ta_pair_lifetime), GPU only.  Every case runs on a float64 AND a
float32 device slab holding the same values and asserts the kernels in the kernel timeline and that no widening kernel ran,
the found lists, run lengths, bonded counts and (fft = 0) lag sums EQUAL to pair_ref's, repeat runs bit-equal, the staged
slab's bits (padding included) unchanged, and the host-facing entry bit-equal to the staged one.

  find    the (Na, Nb) of test_vanhove_distinct_shapes.TILE_CASES (disjoint lists) with 2 frames; every pair bonded, no pair
          bonded (n_pairs == 0); the 64-b-item word edges Nb = 63, 64, 65 and one list of 65 items against itself; searched
          frames in chunks of 1, 2 and all at once.
  series  explicit pairs, P = 1, 2, 3, 129 (odd counts reach the phantom column), T = 1, 2, 3, 7, 63, 64, 65, 1023, 1024, 1025,
  runs    2049, constructed bit patterns: always bonded (one run of T), never bonded, alternating, a single run covering
          exactly frames [63, 65], [1023, 1025] and [0, T - 1] (clipped to the frames there are); "pair_chunk" 1, 2, automatic.
  walk    the two visitors of the shared tile walk (pair_tile.hpp) against each other on exact inputs: the pairs k_pair_find
          finds below r_cut = n_bins dr are the pairs k_vhd_pairs bins below its last edge.
  A small call straight after a large one on one context without ta_trim; float64 positions off any grid in a non-dyadic box:
  everything equal to the CPU backend's; n_atoms dim >= 2^31 is refused before anything is allocated."""
import functools

import numpy as np
import pytest

import pair_ref as ref
from test_vanhove_distinct_shapes import SLABS, TA, TB, TILE_CASES, run_staged, slab_bits, stage, staged_bits
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu


def timeline(c):
    return [n for n, _ in c.kernel_timeline(4096)]


def run_find(c, dtype, x, r_cut, want, repeat=2, **kw):
    runs = []
    for _ in range(repeat):
        runs.append(c.pair_find(r_cut, **kw))
        names = timeline(c)
        assert "k_vhd_gather" in names and "k_pair_find" in names and "k_pair_count" in names, names
        assert ("k_pair_list" in names) == (runs[-1].shape[0] > 0), names
        assert "k_widen_f32" not in names, names  # the slab is read in its own element type
    assert all(np.array_equal(runs[0], r) for r in runs[1:]), "repeat runs differ"
    got = runs[0]
    assert got.dtype == np.int32 and got.ndim == 2 and got.shape[1] == 2
    if want is not None:
        print(f"    found {got.shape[0]} pairs, expected {want.shape[0]}")
        assert np.array_equal(got, want)
    assert np.array_equal(slab_bits(c, dtype), staged_bits(c, x, dtype)), "the staged slab's bits changed"
    return got


def run_lifetime(c, dtype, x, fft, r_cut, pairs, want, repeat=2, **kw):
    """ta_pair_lifetime_staged into a caller's buffers, `repeat` times, and ta_pair_lifetime: all bit-equal; against want =
    (ci, runs, nb, ...) of pair_ref.sums (None: not compared)"""
    import torch

    T = x.shape[0]
    runs = []
    for _ in range(repeat):
        d_ci = torch.full((T,), -7.0, dtype=torch.float64, device="cuda:0")
        d_runs = torch.full((T + 1,), -7, dtype=torch.int64, device="cuda:0")
        d_nb = torch.full((T,), -7.0, dtype=torch.float64, device="cuda:0")
        c.pair_lifetime_staged(fft, r_cut, pairs, d_ci=d_ci.data_ptr(), d_runs=d_runs.data_ptr(), d_nb=d_nb.data_ptr(), **kw)
        torch.cuda.synchronize()
        runs.append((d_ci.cpu().numpy(), d_runs.cpu().numpy(), d_nb.cpu().numpy()))
        names = timeline(c)
        assert "k_pair_series" in names and "k_pair_runs" in names and "k_pair_reduce" in names, names
        assert "k_widen_f32" not in names, names
    for r in runs[1:]:
        assert all(np.array_equal(p, q) for p, q in zip(runs[0], r)), "repeat runs differ"
    host = c.pair_lifetime(fft, r_cut, pairs, **kw)
    assert all(np.array_equal(p, q) for p, q in zip(runs[0], host)), "the host-facing entry differs from the staged one"
    ci, rl, nb = runs[0]
    if want is not None:
        assert np.array_equal(rl, want[1]), np.flatnonzero(rl != want[1])[:5]
        assert np.array_equal(nb, want[2])
        if fft:
            err = float(np.max(np.abs(ci - want[0])))
            print(f"    fft: max |ci - exact| = {err:.3e}, bound {1e-10 * max(float(want[0][0]), 1.0):.3e}")
            assert err <= 1e-10 * max(float(want[0][0]), 1.0)
        else:
            assert np.array_equal(ci, want[0]), np.flatnonzero(ci != want[0])[:5]
    assert np.array_equal(slab_bits(c, dtype), staged_bits(c, x, dtype)), "the staged slab's bits changed"
    return runs[0]


# ---- find ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tile_case(Na, Nb):
    """2 frames of Na + Nb items in the constant box, a = the first Na, b = the others: computed once for both slab types"""
    x = ref.positions(2, Na + Nb, 3)
    a, b = np.arange(Na), np.arange(Na, Na + Nb)
    dims = ref.dimensions(ref.BOX, 2)
    return x, a, b, dims, ref.found(x, a, b, np.array(ref.BOX), ref.R_CUT, 1).astype(np.int32)


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("Na,Nb", TILE_CASES)
def test_find_tiles(Na, Nb, dtype):
    x, a, b, dims, want = tile_case(Na, Nb)
    c = stage(_lib.Context(0), x, dtype)
    try:
        run_find(c, dtype, x, ref.R_CUT, want, idx_a=a, idx_b=b, dimensions=dims)
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_find_all_and_none(dtype):
    """all items on one point: every pair is bonded (Na Nb of two lists, A (A - 1) / 2 of one); items 100 apart: none is"""
    T, A = 3, TB + 5
    one = np.full((T, A, 3), 1.25)
    far = np.zeros((T, A, 3))
    far[:, :, 0] = 100.0 * np.arange(A)[None, :]
    a, b = np.arange(0, TA + 1), np.arange(TA + 1, A)
    c = _lib.Context(0)
    try:
        stage(c, one, dtype)
        got = run_find(c, dtype, one, 0.5, None, idx_a=a, idx_b=b)
        assert np.array_equal(got, np.stack(np.meshgrid(a, b, indexing="ij"), axis=-1).reshape(-1, 2))
        got = run_find(c, dtype, one, 0.5, None, dimensions=ref.dimensions(ref.BOX, T))
        i, j = np.triu_indices(A, k=1)
        assert np.array_equal(got, np.stack([i, j], axis=1))
        stage(c, far, dtype)
        for kw in ({}, dict(idx_a=a, idx_b=b)):
            got = run_find(c, dtype, far, 0.5, None, **kw)
            assert got.shape == (0, 2)
            with pytest.raises(_lib.TAError, match="the found pair list is empty") as e:
                c.pair_lifetime(0, 0.5, None)
            assert e.value.code == -4
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("Nb", [63, 64, 65])
def test_find_word_edges(Nb, dtype):
    """3 a-items against Nb b-items, and Nb + 3 items against themselves, over 7 frames, every third searched"""
    T, A = 7, Nb + 3
    x = ref.positions(T, A, 3)
    dims = ref.dimensions(ref.FRAME_BOXES, T)
    a, b = np.arange(3), np.arange(3, A)
    c = stage(_lib.Context(0), x, dtype)
    try:
        run_find(c, dtype, x, ref.R_CUT, ref.found(x, a, b, dims[:, :3], ref.R_CUT, 3), idx_a=a, idx_b=b, dimensions=dims,
                 search_stride=3)
        run_find(c, dtype, x, ref.R_CUT, ref.found(x, None, None, dims[:, :3], ref.R_CUT, 3), dimensions=dims, search_stride=3)
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_find_chunks_give_the_same_list(dtype):
    x, a, b, dims, axes, pairs, _ = ref.case(7, 70, 3, "disjoint", "frames", 1)
    c = stage(_lib.Context(0), x, dtype)
    try:
        for chunk, launches in ((1, 7), (2, 4), (0, 1), (64, 1)):
            c.set_option("pair_find_chunk", chunk)
            run_find(c, dtype, x, ref.R_CUT, pairs.astype(np.int32), repeat=1, idx_a=a, idx_b=b, dimensions=dims, axes=axes)
            assert c.kernel_launches("k_vhd_gather") == launches == c.kernel_launches("k_pair_find")
    finally:
        c.close()


# ---- the shared tile walk: both visitors on the same exact inputs -----------------------------------------------------------
WALK_BINS, WALK_DR, WALK_BOX = 12, 0.25, 16.0  # r_cut = 12 * 0.25 = 3: fl(r_cut^2) = 9 is the last squared edge (12 * 0.25)^2


@functools.lru_cache(maxsize=None)
def walk_case(D, lists, boxed):
    """2 frames of integer positions in [0, 16]: exact in float32, every r2 an exact integer with or without the box of 16.
    lists "same": one list of TB + 1 items; "disjoint": TA + 1 a-items and TB + 1 b-items, one past each tile edge.  Returns
    x, a, b (None: all items), dimensions and the (n, 2) pairs of frame 0 below r_cut by a NumPy all-pairs compare."""
    Na, Nb = (TB + 1, TB + 1) if lists == "same" else (TA + 1, TB + 1)
    A = Nb if lists == "same" else Na + Nb
    x = np.random.default_rng(100 * D + A).integers(0, 17, size=(2, A, D)).astype(np.float64)
    a, b = (None, None) if lists == "same" else (np.arange(Na), np.arange(Na, A))
    ia, ib = (np.arange(A), np.arange(A)) if lists == "same" else (a, b)
    d = x[0, ib][None, :, :] - x[0, ia][:, None, :]
    if boxed:
        d -= np.rint(d / WALK_BOX) * WALK_BOX
    near = (d * d).sum(axis=2) < (WALK_BINS * WALK_DR) ** 2
    if lists == "same":
        near = np.triu(near, k=1)
    p, q = np.nonzero(near)  # (row-major: sorted by (a, b))
    return x, a, b, ref.dimensions((WALK_BOX,) * 3, 2) if boxed else None, np.stack([ia[p], ib[q]], axis=1).astype(np.int32)


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("lists", ["same", "disjoint"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_walk_visitors_agree(D, lists, dtype):
    """one searched frame (both strides = T) at lag 0: the pair count of ta_pair_find (twice it for one list: the histogram
    counts ordered pairs) equals the sum of ta_vanhove_distinct's non-overflow bins, and the found list is NumPy's"""
    for boxed in (False, True):
        x, a, b, dims, want = walk_case(D, lists, boxed)
        T = x.shape[0]
        c = stage(_lib.Context(0), x, dtype)
        try:
            got = run_find(c, dtype, x, WALK_BINS * WALK_DR, want, repeat=1, search_stride=T, idx_a=a, idx_b=b, dimensions=dims)
            cnt = run_staged(c, [0], WALK_BINS, WALK_DR, repeat=1, origin_stride=T, idx_a=a, idx_b=b, dimensions=dims)
            assert "k_vhd_pairs" in timeline(c)
            n_in = int(cnt[0, :WALK_BINS].sum())
            print(f"    D={D} {lists} boxed={boxed}: {got.shape[0]} pairs found, {n_in} binned below the last edge")
            assert got.shape[0] > 100 and n_in == (2 if lists == "same" else 1) * got.shape[0]
            assert int(cnt[0].sum()) == (x.shape[1] * (x.shape[1] - 1) if lists == "same" else a.size * b.size)
        finally:
            c.close()


# ---- series and runs ------------------------------------------------------------------------------------------------------
PATTERNS = ("always", "never", "alternating", (63, 65), (1023, 1025), "whole")
TS = [1, 2, 3, 7, 63, 64, 65, 1023, 1024, 1025, 2049]


@functools.lru_cache(maxsize=None)
def pattern_sums(T):
    """(bits (6, T), [pair_ref.sums of each pattern alone]): the sums of a call add up over its pairs"""
    bits = np.stack([ref.pattern((0, T - 1) if name == "whole" else name, T) for name in PATTERNS])
    return bits, [ref.sums(row[None, :]) for row in bits]


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T", TS)
def test_series_and_runs_of_constructed_patterns(T, dtype):
    bits6, sums6 = pattern_sums(T)
    c = _lib.Context(0)
    try:
        for P, shifts in ((1, range(6)), (2, range(6)), (3, range(6)), (129, (1,))):
            for shift in shifts:
                which = (np.arange(P) + shift) % 6
                x, pairs = ref.pattern_positions(bits6[which])
                want = [sum(sums6[k][i] for k in which) for i in range(3)]
                stage(c, x, dtype)
                for fft in (0, 1):
                    run_lifetime(c, dtype, x, fft, 0.5, pairs, want, repeat=2 if shift == 1 else 1)
        # a run of T frames is one entry runs[T]; the alternating series has ceil(T / 2) runs of one frame
        assert sums6[0][1][T] == 1 and sums6[2][1][1] == (T + 1) // 2
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_pair_chunks_bit_equal(dtype):
    T, P = 1025, 129
    bits6, sums6 = pattern_sums(T)
    which = np.arange(P) % 6
    x, pairs = ref.pattern_positions(bits6[which])
    want = [sum(sums6[k][i] for k in which) for i in range(3)]
    c = stage(_lib.Context(0), x, dtype)
    try:
        runs = []
        for chunk, launches in ((1, 129), (2, 65), (0, 1), (1000, 1)):
            c.set_option("pair_chunk", chunk)
            runs.append(run_lifetime(c, dtype, x, 0, 0.5, pairs, want, repeat=1))
            assert c.kernel_launches("k_pair_series") == launches == c.kernel_launches("k_pair_runs")
        for r in runs[1:]:
            assert all(np.array_equal(p, q) for p, q in zip(runs[0], r))
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("D", [1, 2, 3])
def test_walks_boxes_and_the_found_list(D, dtype):
    """walks of 65 frames: the search and then ta_pair_lifetime on the list it left in the context (h_pairs NULL), without a
    box, in the constant box and in per-frame boxes; D = 2 on the box axes {0, 2}, D = 1 on axis 1"""
    for boxed in (False, True, "frames"):
        x, a, b, dims, axes, pairs, sums = ref.case(65, 40, D, "same", boxed, 2)
        c = stage(_lib.Context(0), x, dtype)
        try:
            run_find(c, dtype, x, ref.R_CUT, pairs.astype(np.int32), repeat=1, dimensions=dims, axes=axes, search_stride=2)
            if sums is not None:
                run_lifetime(c, dtype, x, 0, ref.R_CUT, None, sums, dimensions=dims, axes=axes)
                run_lifetime(c, dtype, x, 0, ref.R_CUT, pairs, sums, repeat=1, dimensions=dims, axes=axes)
        finally:
            c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_stale_scratch(dtype):
    """a small call, a larger one, then the small one again on ONE context without ta_trim: the second outgrows the first one's
    scratch, bitmap, list and block, the third lies where the second left values"""
    c = _lib.Context(0)
    try:
        for T, A in ((7, 70), (101, 120), (7, 70)):
            x, a, b, dims, axes, pairs, sums = ref.case(T, A, 3, "same", True, 1)
            stage(c, x, dtype)
            run_find(c, dtype, x, ref.R_CUT, pairs.astype(np.int32), repeat=1, dimensions=dims, axes=axes)
            run_lifetime(c, dtype, x, 0, ref.R_CUT, None, sums, repeat=1, dimensions=dims, axes=axes)
    finally:
        c.close()


def test_gpu_equals_cpu_backend():
    """float64 values off any grid (a walk of normal steps, left unwrapped) in the non-dyadic box (3.3, 2.9, 4.1): both backends
    follow pair_math.hpp, so the found list, runs, and ci and nb with fft = 0 are equal -- no tolerance, no excluded pairs"""
    rng = np.random.default_rng(17)
    T, A, D = 9, 700, 3
    x = np.cumsum(rng.normal(scale=0.3, size=(T, A, D)), axis=0) + rng.uniform(0, 50, size=(1, A, D))
    a, b = np.arange(0, A, 2), np.arange(1, A, 2)
    kw = dict(dimensions=ref.dimensions((3.3, 2.9, 4.1), T))
    cpu = _lib.Context("cpu")
    c = stage(_lib.Context(0), x, np.float64)
    try:
        (view,) = cpu.stage_alloc(T, A, D, dtype=np.float64)
        view[:] = x
        cpu.stage_commit(0, T)
        for lists in (dict(idx_a=a, idx_b=b), {}):
            want = cpu.pair_find(1.4, search_stride=2, **lists, **kw)
            got = run_find(c, np.float64, x, 1.4, None, search_stride=2, **lists, **kw)
            assert want.shape[0] > 10000 and np.array_equal(got, want)
            w_ci, w_runs, w_nb = cpu.pair_lifetime(0, 1.4, None, **kw)
            ci, runs, nb = run_lifetime(c, np.float64, x, 0, 1.4, None, None, **kw)
            assert np.array_equal(runs, w_runs) and np.array_equal(ci, w_ci) and np.array_equal(nb, w_nb)
    finally:
        c.close()
        cpu.close()


def test_refuses_2_pow_31_columns():
    """n_atoms dim >= 2^31: TA_E_INVALID before anything is allocated or written.  The slab is device-only, one frame of
    2^30 items x 2 float32 columns (never filled).  "fail_alloc_after" 1 makes the call's first workspace request fail with
    TA_E_NOMEM: the refusal comes first, so no workspace was asked for."""
    import torch

    c = _lib.Context(0)
    try:
        c.set_option("stage_device_f32", 1)
        c.stage_alloc_device(1, 2 ** 30, 2)
        out = torch.full((2,), -7, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        c.set_option("fail_alloc_after", 1)
        with pytest.raises(_lib.TAError, match="pair_lifetime: n_atoms \\* dim must be below 2\\^31") as e:
            c.pair_lifetime_staged(0, 0.5, np.array([[0, 1]]), d_runs=out.data_ptr())
        assert e.value.code == -1
        with pytest.raises(_lib.TAError, match="pair_find: n_atoms \\* dim must be below 2\\^31") as e:
            c.pair_find(0.5, idx_a=[0, 1], idx_b=[2])
        assert e.value.code == -1
        c.set_option("fail_alloc_after", 0)
        torch.cuda.synchronize()
        assert bool((out == -7).all())
    finally:
        c.close()
