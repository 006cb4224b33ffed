"""k_vhd_gather and k_vhd_pairs at shapes that reach every branch, through the C-ABI (ta_vanhove_distinct_staged,
ta_vanhove_distinct), GPU only.  Every case runs on a float64 AND a float32 device slab holding the same values and asserts
both kernels in the kernel timeline and that no widening kernel ran, the counts EQUAL to vanhove_distinct_ref's, repeat runs
bit-equal, the staged slab's bits (padding included) unchanged, and the host-facing entry bit-equal to the staged one.

With the pair kernel's tiles TA = 256 a-items and TB = 1024 b-items per workgroup:
  * one item, a tile short of one, a full tile, a tail of one, two tiles and a tail, on each side;
  * 1, 2, 3 frames with 1 and 2 items; an odd frame count with odd and even lags (the gather's last row is row T - 1);
  * origin strides 1, 3, 7 over 101 frames; D = 1, D = 2 on the box axes {0, 2}, D = 3;
  * no box, a constant box, per-frame boxes at lag 0; 1, 50 and 4096 bins;
  * every pair in overflow, every pair in bin 0; a small call straight after a large one on one context;
  * lags in chunks of 1, 2 and all at once: the same bits;
  * float64 positions off any grid in a non-dyadic box: the GPU's counts equal the CPU backend's exactly;
  * n_atoms dim >= 2^31 is refused before anything is allocated."""
import ctypes

import numpy as np
import pytest

import vanhove_distinct_ref as ref
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu

SLABS = [pytest.param(np.float64, id="slab64"), pytest.param(np.float32, id="slab32")]
TA, TB = 256, 1024


def stage(c, x, dtype):
    """x staged in `dtype` on context c (replacing what it held), kept in that element type on the device"""
    T, A, D = x.shape
    c.set_option("stage_device_f32", int(dtype == np.float32))
    (view,) = c.stage_alloc(T, A, D, dtype=dtype)
    view[:] = x
    c.stage_commit(0, T)
    c.set_option("timeline", 1)
    return c


def run_staged(c, lags, n_bins, dr, repeat=2, **kw):
    """ta_vanhove_distinct_staged into a caller's buffer, `repeat` times: the runs must agree bit for bit"""
    import torch

    runs = []
    for _ in range(repeat):
        cnt = torch.full((len(lags), n_bins + 1), -7, dtype=torch.int64, device="cuda:0")
        c.vanhove_distinct_staged(lags, n_bins, dr, cnt.data_ptr(), **kw)
        torch.cuda.synchronize()
        runs.append(cnt.cpu().numpy())
    assert all(np.array_equal(runs[0], r) for r in runs[1:]), "repeat runs differ"
    return runs[0]


def slab_bits(c, dtype):
    """the raw staged device slab, padding included, read after the calls on it have completed"""
    ptr, pitch, n_pairs = c.stage_device(0)
    raw = np.empty(n_pairs * pitch * 2, dtype=dtype)
    L = _lib.lib()
    L.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert L.hipMemcpy(raw.ctypes.data, ptr, raw.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return raw.view(np.uint32 if dtype == np.float32 else np.uint64)


def staged_bits(c, x, dtype):
    """what the slab holds when nothing has touched it since staging: the pair-major layout of x in `dtype`, rows
    T ... pitch - 1 and the phantom column of an odd column count zero"""
    T, A, D = x.shape
    _, pitch, n_pairs = c.stage_device(0)
    want = np.zeros((n_pairs * 2, pitch), dtype=dtype)
    want[:A * D, :T] = x.reshape(T, A * D).T
    want = want.reshape(n_pairs, 2, pitch).transpose(0, 2, 1)
    return np.ascontiguousarray(want).ravel().view(np.uint32 if dtype == np.float32 else np.uint64)


def check(c, dtype, x, lags, bins, want, what="", **kw):
    """one call through both entries against `want` (None: not compared), with everything the module's docstring lists"""
    got = run_staged(c, lags, *bins, **kw)
    names = [n for n, _ in c.kernel_timeline(64)]
    assert "k_vhd_gather" in names and "k_vhd_pairs" in names, names
    assert "k_widen_f32" not in names, names  # the slab is read in its own element type
    if want is not None:
        ref.assert_counts(got, want, what=f"{what} bins={bins}")
    host = c.vanhove_distinct(lags, *bins, **kw)
    assert np.array_equal(host, got), "the host-facing entry differs from the staged one"
    assert np.array_equal(slab_bits(c, dtype), staged_bits(c, x, dtype)), "the staged slab's bits changed"
    return got


def check_case(dtype, case, stride, what):
    x, lags, a, b, dims, axes, refs = case
    c = stage(_lib.Context(0), x, dtype)
    try:
        for bins in ref.BINS:
            check(c, dtype, x, lags, bins, refs[bins], what, origin_stride=stride, idx_a=a, idx_b=b, dimensions=dims, axes=axes)
    finally:
        c.close()


# (Na, Nb): a = the first Na items, b = the last Nb of max(Na, Nb) + 3 items (they overlap unless one of them is tiny)
TILE_CASES = [(1, 1), (TA - 1, TB + 1), (TA, TB), (TA + 1, TB - 1), (2 * TA + 3, 2 * TB + 3), (1, 2 * TB + 3), (2 * TA + 3, 1),
              (TB + 1, TA - 1)]


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("Na,Nb", TILE_CASES)
def test_tiles(Na, Nb, dtype):
    """2 frames, lags 0 and 1, the constant box: at most 3 (2 TA + 3) (2 TB + 3) = 3.2e6 pairs"""
    A = max(Na, Nb) + 3
    x = ref.positions(2, A, 3)
    a, b = np.arange(Na), np.arange(A - Nb, A)
    lags = np.array([0, 1])
    dims = ref.dimensions(ref.BOX, 2)
    c = stage(_lib.Context(0), x, dtype)
    try:
        for bins in ref.BINS:
            want = tile_reference(Na, Nb, bins)
            got = check(c, dtype, x, lags, bins, want, f"Na={Na} Nb={Nb}", idx_a=a, idx_b=b, dimensions=dims)
            assert np.array_equal(got.sum(axis=1), np.array([2, 1]) * (Na * Nb - np.intersect1d(a, b).size))
    finally:
        c.close()


_tile_refs = {}


def tile_reference(Na, Nb, bins):
    """computed once and shared by the two slab variants"""
    if (Na, Nb) not in _tile_refs:
        A = max(Na, Nb) + 3
        _tile_refs[Na, Nb] = dict(zip(ref.BINS, ref.references(ref.positions(2, A, 3), [0, 1], 1, np.arange(Na), np.arange(A - Nb, A),
                                                               np.array(ref.BOX), ref.BINS)))
    return _tile_refs[Na, Nb][bins]


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T,A", [(1, 1), (2, 1), (3, 1), (1, 2), (2, 2), (3, 2)])
def test_few_frames_few_items(T, A, dtype):
    for boxed in (False, True):
        check_case(dtype, ref.case(T, A, 3, 1, "same", boxed), 1, f"T={T} A={A} box={boxed}")


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("D", [1, 2, 3])
def test_odd_frames_odd_and_even_lags(D, dtype):
    """7 frames, lags 0, 1, 2, 3, 6: the lagged rows of both parities, the last one row T - 1 of an odd T; D = 2 on the box
    axes {0, 2}, D = 1 on axis 1"""
    for boxed in (False, True):
        check_case(dtype, ref.case(7, 70, D, 1, "overlap", boxed), 1, f"D={D} box={boxed}")
    check_case(dtype, ref.case(7, 70, D, 2, "disjoint", "frames"), 2, f"D={D} per-frame boxes")


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("stride", [1, 3, 7])
def test_origin_strides(stride, dtype):
    """101 frames: 101, 34 and 15 origins at lag 0, fewer at the lags 1, 2, 50, 100"""
    check_case(dtype, ref.case(101, 40, 3, stride, "overlap", True), stride, f"stride={stride}")


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("n_bins,dr", [(1, 1.0), (50, 0.02), (4096, 1.0 / 4096)])
def test_bin_counts(n_bins, dr, dtype):
    x, lags, a, b, dims, axes, _ = ref.case(7, 70, 3, 1, "overlap", True)
    want = ref.reference(x, lags, 1, a, b, np.array(ref.BOX), n_bins, dr)
    c = stage(_lib.Context(0), x, dtype)
    try:
        check(c, dtype, x, lags, (n_bins, dr), want, f"B={n_bins}", idx_a=a, idx_b=b, dimensions=dims, axes=axes)
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_all_overflow_and_all_bin_0(dtype):
    """items 100 apart without a box: every pair is overflow; all items on one point: every pair is in bin 0"""
    T, A = 3, TB + 5
    far = np.zeros((T, A, 3))
    far[:, :, 0] = 100.0 * np.arange(A)[None, :]
    one = np.full((T, A, 3), 1.25)
    lags, n_pairs = np.array([0, 2]), np.array([3, 1]) * A * (A - 1)
    for x, column, kw in ((far, 8, {}), (one, 0, {}), (one, 0, {"dimensions": ref.dimensions(ref.BOX, T)})):
        c = stage(_lib.Context(0), x, dtype)
        try:
            want = np.zeros((2, 9), dtype=np.int64)
            want[:, column] = n_pairs
            check(c, dtype, x, lags, (8, 0.125), want, f"column {column}", **kw)
        finally:
            c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_stale_scratch(dtype):
    """A small call (7 frames, 70 items), a larger one (101 frames, 300 items, 5 lags), then the small one again, on ONE context
    without ta_trim: the second call outgrows the first one's scratch, histogram and table, the third lies where the second
    left values"""
    c = _lib.Context(0)
    try:
        for T, A, stride in ((7, 70, 1), (101, 300, 7), (7, 70, 1)):
            x, lags, a, b, dims, axes, refs = ref.case(T, A, 3, stride, "overlap", True)
            stage(c, x, dtype)
            for bins in ref.BINS:
                check(c, dtype, x, lags, bins, refs[bins], f"T={T}", origin_stride=stride, idx_a=a, idx_b=b, dimensions=dims,
                      axes=axes)
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_chunks_bit_equal(dtype):
    x, lags, a, b, dims, axes, refs = ref.case(101, 40, 3, 3, "overlap", True)
    assert len(lags) == 5
    kw = dict(origin_stride=3, idx_a=a, idx_b=b, dimensions=dims, axes=axes)
    c = stage(_lib.Context(0), x, dtype)
    try:
        for bins in ref.BINS:
            runs = []
            for chunk, launches in ((1, 5), (2, 3), (0, 1), (64, 1)):
                c.set_option("vanhove_distinct_chunk", chunk)
                runs.append(run_staged(c, lags, *bins, repeat=1, **kw))
                assert c.kernel_launches("k_vhd_gather") == launches == c.kernel_launches("k_vhd_pairs")
            assert all(np.array_equal(runs[0], r) for r in runs[1:]), bins
            ref.assert_counts(runs[0], refs[bins], what=f"chunks bins={bins}")
    finally:
        c.close()


def test_gpu_counts_equal_cpu_backend():
    """float64 values off any grid (a walk of normal steps, left unwrapped) in the non-dyadic box (3.3, 2.9, 4.1): both backends
    follow vanhove_distinct_math.hpp, so the counts are equal -- no tolerance, no reference, no excluded pairs"""
    rng = np.random.default_rng(17)
    T, A, D = 9, 700, 3
    x = np.cumsum(rng.normal(scale=0.3, size=(T, A, D)), axis=0) + rng.uniform(0, 50, size=(1, A, D))
    lags = ref.lag_sample(T)
    a, b = ref.index_lists("overlap", A)
    kw = dict(origin_stride=2, idx_a=a, idx_b=b, dimensions=ref.dimensions((3.3, 2.9, 4.1), T))
    n_bins, dr = 50, 1.45 / 50
    cpu = _lib.Context("cpu")
    c = stage(_lib.Context(0), x, np.float64)
    try:
        (view,) = cpu.stage_alloc(T, A, D, dtype=np.float64)
        view[:] = x
        cpu.stage_commit(0, T)
        want = cpu.vanhove_distinct(lags, n_bins, dr, **kw)
        got = check(c, np.float64, x, lags, (n_bins, dr), None, **kw)
        assert want[:, -1].sum() > 0 and want[:, :-1].sum() > 100000
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
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
        cnt = torch.full((1, 5), -7, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        c.set_option("fail_alloc_after", 1)
        with pytest.raises(_lib.TAError, match="n_atoms \\* dim must be below 2\\^31") as e:
            c.vanhove_distinct_staged([0], 4, 0.5, cnt.data_ptr())
        assert e.value.code == -1
        c.set_option("fail_alloc_after", 0)
        torch.cuda.synchronize()
        assert bool((cnt == -7).all())
    finally:
        c.close()
