"""k_vanhove at shapes that reach every branch, through the C-ABI (ta_vanhove_staged, ta_vanhove_dev, ta_group_vanhove),
GPU only.  Every shape runs on a float64 AND a float32 device slab holding the same values, with lags = lag_sample(T) and
both binnings of vanhove_ref.BINS, asserts k_vanhove in the kernel timeline and that no widening kernel ran, that repeat
runs agree bit for bit in counts AND moments, that the staged slab's bits (padding included) are unchanged, and compares
with vanhove_ref: the counts EQUAL, the moments within 1e-10 relative.

  * column pairs that straddle atoms with an odd column count (D = 3, odd A), D = 2 and D = 1;
  * 1, 2, 3 frames with 1 and 2 atoms; an odd frame count over two frame blocks (lagged float32 rows at odd and even lags,
    the float32 load whose second row is row T);
  * more atoms than pm_unit_grid gives groups at one frame block (units loop); eleven frame blocks with lags up to T - 1
    crossing them;
  * five lags in chunks of 1, 2 and all at once: the same bits, and 5, 3, 1 launches of k_vanhove; 4096 and 3000 bins, where
    the LDS formula of DESIGN 4.15 gives 1 and 3 lags per launch;
  * a smaller call straight after a larger one on the same context (the scratch histogram and partials are rewritten);
  * the frame-major entry against the staged one bit for bit; two group members on one GPU with an odd split;
  * non-grid float64 values: the GPU's counts equal the CPU backend's exactly."""
import ctypes

import numpy as np
import pytest

import vanhove_ref as ref
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


def run_staged(c, lags, n_bins, dr, repeat=2, counts=True, moments=True):
    """ta_vanhove_staged into caller buffers, `repeat` times: the runs must agree bit for bit.  -> (counts, moments)"""
    import torch

    dev = torch.device("cuda", 0)
    L = len(lags)
    runs = []
    for _ in range(repeat):
        cnt = torch.full((L, n_bins + 1), -7, dtype=torch.int64, device=dev)
        mom = torch.full((L, 2), np.nan, dtype=torch.float64, device=dev)
        c.vanhove_staged(lags, n_bins, dr, cnt.data_ptr() if counts else 0, mom.data_ptr() if moments else 0)
        torch.cuda.synchronize()
        runs.append((cnt.cpu().numpy() if counts else None, mom.cpu().numpy() if moments else None))
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


def check(c, dtype, case, what=""):
    x, lags, refs = case
    out = {}
    for bins in ref.BINS:
        cnt, mom = run_staged(c, lags, *bins)
        names = timeline(c)
        assert "k_vanhove" in names, names
        assert "k_widen_f32" not in names, names  # the slab is read in its own element type
        ref.assert_vanhove(cnt, mom, refs[bins], what=f"{what} bins={bins}")
        out[bins] = (cnt, mom)
    assert np.array_equal(slab_bits(c, dtype), staged_bits(c, x, dtype)), "the staged slab's bits changed"
    return out


def units_loop_atoms():
    """more atoms than pm_unit_grid gives groups at one frame block: 16 groups per CU"""
    import torch

    return max(5001, 16 * torch.cuda.get_device_properties(0).multi_processor_count + 905)


# (id, T, A, D); A None: units_loop_atoms()
SHAPE_CASES = [
    ("straddle", 100, 1501, 3),
    ("d2", 65, 1100, 2),
    ("d1", 513, 2101, 1),
    ("t1a1", 1, 1, 3), ("t2a1", 2, 1, 3), ("t3a1", 3, 1, 3),
    ("t1a2", 1, 2, 3), ("t2a2", 2, 2, 3), ("t3a2", 3, 2, 3),
    ("two_frame_blocks", 1101, 300, 3),
    ("units_loop", 48, None, 3),
    ("long", 10300, 33, 3),
]


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T,A,D", [pytest.param(*c[1:], id=f"{c[0]}-T{c[1]}-A{c[2]}-D{c[3]}") for c in SHAPE_CASES])
def test_vanhove_shapes(T, A, D, dtype):
    case = ref.case(T, A or units_loop_atoms(), D)
    c = stage(_lib.Context(0), case[0], dtype)
    try:
        got = check(c, dtype, case)
        bins = ref.BINS[0]
        host = c.vanhove(case[1], *bins)  # the host-facing call
        assert all(np.array_equal(a, b) for a, b in zip(host, got[bins]))
        only_counts = run_staged(c, case[1], *bins, repeat=1, moments=False)
        only_moments = run_staged(c, case[1], *bins, repeat=1, counts=False)
        assert np.array_equal(only_counts[0], got[bins][0]) and np.array_equal(only_moments[1], got[bins][1])
    finally:
        c.close()


def lds_chunk(n_bins):
    """the lags per launch that fit 64 KiB of LDS -- e[B + 1] doubles, per lag 4 waves x 2 doubles and B + 1 uint32"""
    return max(1, (65536 - 8 * (n_bins + 1)) // (64 + 4 * (n_bins + 1)))


@pytest.mark.parametrize("dtype", SLABS)
def test_vanhove_chunks_bit_equal(dtype):
    x, lags, refs = ref.case(100, 301, 3)
    pick = [0, 1, 4, 6, 10]  # lags 0, 1, 7, 63, 99
    lags5 = np.ascontiguousarray(lags[pick])
    c = stage(_lib.Context(0), x, dtype)
    try:
        for bins in ref.BINS:
            runs = []
            for chunk, launches in ((1, 5), (2, 3), (0, 1)):
                c.set_option("vanhove_chunk", chunk)
                runs.append(run_staged(c, lags5, *bins, repeat=1))
                assert c.kernel_launches("k_vanhove") == launches, (chunk, c.kernel_launches("k_vanhove"))
            for r in runs[1:]:
                assert all(np.array_equal(a, b) for a, b in zip(runs[0], r)), bins
            want = refs[bins]
            ref.assert_vanhove(*runs[0], (want[0][pick], want[1][pick]), what=f"chunks bins={bins}")
        # many bins: the automatic chunk is what fits the LDS, fewer lags than the call has
        for n_bins, dr in ((4096, 1.0 / 512), (3000, 0.003)):
            fit = lds_chunk(n_bins)
            assert fit < 5 and fit == {4096: 1, 3000: 3}[n_bins]
            c.set_option("vanhove_chunk", 0)
            auto = run_staged(c, lags5, n_bins, dr, repeat=1)
            assert c.kernel_launches("k_vanhove") == -(-5 // fit) > 1
            c.set_option("vanhove_chunk", 64)  # more than fit: what fits
            capped = run_staged(c, lags5, n_bins, dr, repeat=1)
            assert c.kernel_launches("k_vanhove") == -(-5 // fit)
            c.set_option("vanhove_chunk", 1)
            ones = run_staged(c, lags5, n_bins, dr, repeat=1)
            assert c.kernel_launches("k_vanhove") == 5
            for r in (capped, ones):
                assert all(np.array_equal(a, b) for a, b in zip(auto, r)), n_bins
            ref.assert_vanhove(*auto, ref.reference(x, lags5, n_bins, dr), what=f"B={n_bins}")
    finally:
        c.close()


def test_vanhove_stale_scratch():
    """A larger call (1101 frames, 300 atoms, 15 lags) then a smaller one (99 frames, 150 atoms, 11 lags) on ONE context
    without ta_trim: the second call's histogram and partials lie where the first left values."""
    c = _lib.Context(0)
    try:
        for T, A in ((1101, 300), (99, 150)):
            case = ref.case(T, A, 3)
            stage(c, case[0], np.float64)
            check(c, np.float64, case, what=f"T={T}")
    finally:
        c.close()


def test_vanhove_dev_wide_rows():
    """ta_vanhove_dev on a frame-major tensor with ld_row > n_atoms dim equals the staged path bit for bit"""
    import torch

    x, lags, refs = ref.case(1101, 300, 3)
    T, A, D = x.shape
    ld_row = A * D + 7
    wide = np.full((T, ld_row), 7.5e3)
    wide[:, :A * D] = x.reshape(T, A * D)
    d_x = torch.from_numpy(wide).to("cuda:0")
    c = stage(_lib.Context(0), x, np.float64)
    try:
        for bins in ref.BINS:
            want = run_staged(c, lags, *bins)
            cnt = torch.full((len(lags), bins[0] + 1), -7, dtype=torch.int64, device="cuda:0")
            mom = torch.full((len(lags), 2), np.nan, dtype=torch.float64, device="cuda:0")
            c.vanhove_dev(d_x.data_ptr(), T, A, D, ld_row, lags, *bins, cnt.data_ptr(), mom.data_ptr())
            torch.cuda.synchronize()
            names = timeline(c)
            assert "k_relayout" in names and "k_vanhove" in names, names
            for a, b in zip(want, (cnt, mom)):
                assert np.array_equal(a, b.cpu().numpy()), bins
    finally:
        c.close()


def test_group_vanhove():
    """ta_group_vanhove on devices [0, 0] (751 + 750 atoms: an odd split) against one context: the members' counts add up
    exactly, their moments within the bar"""
    x, lags, refs = ref.case(100, 1501, 3)
    T, A, D = x.shape
    bins = ref.BINS[1]
    c = stage(_lib.Context(0), x, np.float64)
    g = _lib.Group([0, 0])
    try:
        one = c.vanhove(lags, *bins)
        (views,) = g.stage_alloc(T, A, D)
        assert any((hi - lo) % 2 for lo, hi in g.shards)
        for (lo, hi), view in zip(g.shards, views):
            view[:] = x[:, lo:hi]
        g.stage_commit(0, T)
        cnt, mom = g.vanhove(lags, *bins)
        assert np.array_equal(cnt, one[0])
        ref.assert_vanhove(cnt, mom, refs[bins], what="group")
        only = g.vanhove(lags, *bins, moments=False)
        assert only[1] is None and np.array_equal(only[0], cnt)
        assert np.array_equal(g.vanhove(lags, *bins, counts=False)[1], mom)
    finally:
        g.close()
        c.close()


def test_vanhove_gpu_counts_equal_cpu_backend():
    """float64 values off any grid (a walk of normal steps): both backends follow the same r2 arithmetic and the same table,
    so the counts are equal -- no tolerance, no excluded pairs"""
    rng = np.random.default_rng(17)
    T, A, D = 100, 1501, 3
    x = np.cumsum(rng.normal(scale=0.3, size=(T, A, D)), axis=0) + rng.uniform(0, 50, size=(1, A, D))
    lags = ref.lag_sample(T)
    n_bins, dr = 50, 0.1
    cpu = _lib.Context("cpu")
    c = stage(_lib.Context(0), x, np.float64)
    try:
        (view,) = cpu.stage_alloc(T, A, D, dtype=np.float64)
        view[:] = x
        cpu.stage_commit(0, T)
        want_c, want_m = cpu.vanhove(lags, n_bins, dr)
        got_c, got_m = run_staged(c, lags, n_bins, dr)
        assert got_c.sum() == A * int((T - lags).sum()) and want_c[:, -1].sum() > 0 and want_c[:, :-1].sum() > 0
        assert np.array_equal(got_c, want_c), np.argwhere(got_c != want_c)[:5]
        scale = np.where(want_m > 0, want_m, 1.0)
        assert np.max(np.abs(got_m - want_m) / scale) <= 1e-10
    finally:
        c.close()
        cpu.close()


def test_vanhove_dev_refuses_2_pow_31_columns():
    """n_atoms dim >= 2^31: TA_E_INVALID from the frame-major entry before anything is read or written (the pointers are
    those of a small tensor: a call that went on would be caught by the sentinels, not by a fault)"""
    import torch

    d_x = torch.zeros(16, dtype=torch.float64, device="cuda:0")
    cnt = torch.full((1, 5), -7, dtype=torch.int64, device="cuda:0")
    c = _lib.Context(0)
    try:
        with pytest.raises(_lib.TAError, match="n_atoms \\* dim must be below 2\\^31") as e:
            c.vanhove_dev(d_x.data_ptr(), 1, 2 ** 30, 2, 2 ** 31, [0], 4, 0.5, cnt.data_ptr())
        assert e.value.code == -1
        torch.cuda.synchronize()
        assert bool((cnt == -7).all())
    finally:
        c.close()
