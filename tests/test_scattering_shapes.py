"""k_phase and the evaluations behind it at shapes that reach every branch, through the C-ABI (ta_scatter_staged,
ta_scatter_dev, ta_group_scatter), GPU only.  Every shape runs with fft 1 and 0 on a float64 AND a float32 device slab
holding the same values, asserts k_phase in the kernel timeline, that no widening kernel ran and that a lag kernel of the
family the VACF dispatch picks for (T, D = 2) did, that repeat runs agree bit for bit, that the staged slab's bits (padding
included) are unchanged, and compares with scatter_ref at lag_sample for every wavevector: the density within its derived
bar, self within 1e-10 of its max, coll within 1e-10 of its max against the long-double autocorrelation of the returned
density.

  * column pairs that straddle atoms with an odd column count (D = 3, odd A), D = 2 and D = 1;
  * 1, 2, 3 frames with 1 and 2 atoms; an odd frame count over two frame blocks (the float32 load whose second row is row T);
  * more atoms than pm_unit_grid gives groups at one frame block (units loop); eleven frame blocks with an outer-radix plan;
  * five wavevectors in chunks of 1, 2 and all at once: the same bits, and 5, 3, 1 launches of k_phase;
  * a smaller call straight after a larger one on the same context (tail rows and blocks are written, not assumed);
  * the frame-major entry against the staged one bit for bit; two group members on one GPU with an odd split."""
import ctypes

import numpy as np
import pytest

import scatter_ref as ref
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu

SLABS = [pytest.param(np.float64, id="slab64"), pytest.param(np.float32, id="slab32")]


def stage(c, x, dtype):
    """x staged in `dtype` on context c (replacing what it held), kept in that element type on the device"""
    T, A, D = x.shape
    c.set_option("stage_device_f32", int(dtype == np.float32))
    (view,) = c.stage_alloc(T, A, D, dtype=dtype)
    view[:] = x
    c.stage_commit(0, T)
    c.set_option("timeline", 1)
    return c


def timeline(c):
    return [n for n, _ in c.kernel_timeline(64)]


def run_staged(c, fft, k, repeat=2, coll=True):
    """ta_scatter_staged into caller buffers, `repeat` times: the runs must agree bit for bit.  -> (self, density, coll)"""
    import torch

    dev = torch.device("cuda", 0)
    T, K = c.shape[0], k.shape[0]
    runs = []
    for _ in range(repeat):
        fs = torch.full((K, T), np.nan, dtype=torch.float64, device=dev)
        rho = torch.full((K, T, 2), np.nan, dtype=torch.float64, device=dev)
        cl = torch.full((K, T), np.nan, dtype=torch.float64, device=dev)
        c.scatter_staged(fft, k, fs.data_ptr(), rho.data_ptr(), cl.data_ptr() if coll else 0)
        torch.cuda.synchronize()
        runs.append((fs.cpu().numpy(), rho.cpu().numpy(), cl.cpu().numpy() if coll else None))
    for r in runs[1:]:
        assert all(a is None or np.array_equal(a, b) for a, b in zip(runs[0], r)), "repeat runs differ"
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


def lag_kernels(T, fft):
    """a kernel only the VACF lag-sum dispatch of this length launches on a float64 slab (api.hip: fft_impl, direct_impl with
    the default options), as tests/test_species_self_shapes.py names them for the VACF self terms"""
    if T <= 48 or (T <= 64 and not fft):
        return {"k_short"}
    if not fft:
        return {"k_mid"} if 97 <= T <= 512 else set()  # (beyond: the matrix-core forms, named by the VACF tests)
    return {"k_w1_accum"} if T <= 512 else {"k_wsplit_accum", "k_winverse"}


def check(c, dtype, case, what=""):
    x, k = case[0], case[1]
    for fft in (1, 0):
        fs, rho, coll = run_staged(c, fft, k)
        names = timeline(c)
        assert "k_phase" in names, names
        assert "k_widen_f32" not in names, names  # the slab is read in its own element type
        assert lag_kernels(x.shape[0], fft) <= set(names), (fft, names)
        ref.assert_scatter(fs, rho, coll, case, what=f"{what} fft={fft}")
    assert np.array_equal(slab_bits(c, dtype), staged_bits(c, x, dtype)), "the staged slab's bits changed"
    return fs, rho, coll


def units_loop_atoms():
    """more atoms than pm_unit_grid gives groups at one frame block: 16 groups per CU"""
    import torch

    return max(5001, 16 * torch.cuda.get_device_properties(0).multi_processor_count + 905)


# (id, T, A, D, K); A None: units_loop_atoms()
SHAPE_CASES = [
    ("straddle", 100, 1501, 3, 3),
    ("d2", 65, 1100, 2, 2),
    ("d1", 513, 2101, 1, 5),
    ("t1a1", 1, 1, 3, 1), ("t2a1", 2, 1, 3, 1), ("t3a1", 3, 1, 3, 1),
    ("t1a2", 1, 2, 3, 1), ("t2a2", 2, 2, 3, 1), ("t3a2", 3, 2, 3, 1),
    ("two_frame_blocks", 1101, 300, 3, 2),
    ("units_loop", 48, None, 3, 2),
    ("outer_radix", 10300, 33, 3, 2),
]


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T,A,D,K", [pytest.param(*c[1:], id=f"{c[0]}-T{c[1]}-A{c[2]}-D{c[3]}-K{c[4]}") for c in SHAPE_CASES])
def test_scatter_shapes(T, A, D, K, dtype):
    case = ref.case(T, A or units_loop_atoms(), D, K)
    c = stage(_lib.Context(0), case[0], dtype)
    try:
        fs, rho, coll = check(c, dtype, case)
        host = c.scatter(0, case[1])  # the host-facing call
        assert all(np.array_equal(a, b) for a, b in zip(host, (fs, rho, coll)))
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_scatter_chunks_bit_equal(dtype):
    case = ref.case(100, 301, 3, 5)
    c = stage(_lib.Context(0), case[0], dtype)
    try:
        for fft in (1, 0):
            runs = []
            for chunk, launches in ((1, 5), (2, 3), (0, 1)):
                c.set_option("scatter_chunk", chunk)
                runs.append(run_staged(c, fft, case[1], repeat=1))
                assert c.kernel_launches("k_phase") == launches, (chunk, c.kernel_launches("k_phase"))
            for r in runs[1:]:
                assert all(np.array_equal(a, b) for a, b in zip(runs[0], r)), fft
            ref.assert_scatter(*runs[0], case, what=f"chunks fft={fft}")
    finally:
        c.close()


def test_scatter_stale_scratch():
    """A larger call (1101 frames, 300 atoms, two wavevectors) then a smaller one (99 frames: rows 99 ... 103 of every pair,
    150 atoms, one wavevector) on ONE context without ta_trim: the second call's phase slab, its tail rows and the
    densities' pair-major copy lie where the first left values."""
    c = _lib.Context(0)
    try:
        for T, A, K in ((1101, 300, 2), (99, 150, 1)):
            case = ref.case(T, A, 3, K)
            stage(c, case[0], np.float64)
            check(c, np.float64, case, what=f"T={T}")
    finally:
        c.close()


def test_scatter_dev_wide_rows():
    """ta_scatter_dev on a frame-major tensor with ld_row > n_atoms dim equals the staged path bit for bit"""
    import torch

    case = ref.case(1101, 300, 3, 2)
    x, k = case[0], case[1]
    T, A, D = x.shape
    ld_row = A * D + 7
    wide = np.full((T, ld_row), 7.5e3)
    wide[:, :A * D] = x.reshape(T, A * D)
    d_x = torch.from_numpy(wide).to("cuda:0")
    c = stage(_lib.Context(0), x, np.float64)
    try:
        for fft in (1, 0):
            want = run_staged(c, fft, k)
            fs = torch.full((2, T), np.nan, dtype=torch.float64, device="cuda:0")
            rho = torch.full((2, T, 2), np.nan, dtype=torch.float64, device="cuda:0")
            cl = torch.full((2, T), np.nan, dtype=torch.float64, device="cuda:0")
            c.scatter_dev(d_x.data_ptr(), T, A, D, ld_row, fft, k, fs.data_ptr(), rho.data_ptr(), cl.data_ptr())
            torch.cuda.synchronize()
            names = timeline(c)
            assert "k_relayout" in names and "k_phase" in names, names
            for a, b in zip(want, (fs, rho, cl)):
                assert np.array_equal(a, b.cpu().numpy()), fft
    finally:
        c.close()


def test_group_scatter():
    """ta_group_scatter on devices [0, 0] (751 + 750 atoms: an odd split) against one context: the members' self parts and
    densities add up within the bars, the collective part is that of the summed density"""
    case = ref.case(100, 1501, 3, 3)
    x, k = case[0], case[1]
    T, A, D = x.shape
    g = _lib.Group([0, 0])
    try:
        (views,) = g.stage_alloc(T, A, D)
        assert any((hi - lo) % 2 for lo, hi in g.shards)
        for (lo, hi), view in zip(g.shards, views):
            view[:] = x[:, lo:hi]
        g.stage_commit(0, T)
        for fft in (1, 0):
            ref.assert_scatter(*g.scatter(fft, k), case, what=f"group fft={fft}")
            fs, rho, coll = g.scatter(fft, k, density=False)  # the density summed inside the call
            assert rho is None
            ref.assert_scatter(fs, None, None, case, what=f"group fft={fft}")
            assert np.array_equal(coll, g.scatter(fft, k, self_part=False)[2])
    finally:
        g.close()
