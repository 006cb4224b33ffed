"""k_species_current and the cross-correlation at shapes that reach every branch of the kernel, through the C-ABI (the
staged and the frame-major device entry points), GPU only.  Every case runs on a float64 AND on a float32 device slab,
asserts k_species_current in the kernel timeline and -- for the float32 slab -- that no widening kernel ran, and compares
the currents at every frame, and C at every lag and for all S^2 pairs, with the long-double references of current_ref:

  * column pairs that straddle two atoms OF DIFFERENT SPECIES (D = 3, labels alternating atom by atom), odd column counts
    (the unpaired last column), D = 2 and D = 1;
  * every species class of the kernel template and both ends of each: S = 1, 2 | 3, 4 | 5, 8 -- on a float32 slab the
    first two load two frames per thread, the third swaps halves between the lanes of a pair;
  * more column pairs than groups of pairs, so one group sums pairs of several species;
  * 1, 2, 3, 1023, 1024, 1025, 2049 and 20000 frames: odd frame counts (the float32 load whose second row is row T),
    partial frame blocks, 20 frame blocks with few groups and an outer-radix FFT plan for C;
  * frame-major input with ld_row > n_atoms dim;
  * the slab's rows T ... pitch - 1 and the phantom column are still zero afterwards.

The velocities are rounded to float32 first, so both slab types hold the same values and share one reference."""
import ctypes
import functools

import numpy as np
import pytest

from current_ref import assert_cross, assert_currents, cross_ref, currents_ref, species_velocities
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu

SLABS = [pytest.param(np.float64, id="slab64"), pytest.param(np.float32, id="slab32")]


def staged_context(v, dtype):
    """the velocities staged in `dtype`, kept in that element type on the device"""
    T, A, D = v.shape
    c = _lib.Context(0)
    c.set_option("stage_device_f32", int(dtype == np.float32))
    (view,) = c.stage_alloc(T, A, D, dtype=dtype)
    view[:] = v
    c.stage_commit(0, T)
    c.set_option("timeline", 1)
    return c


def timeline(c):
    return [n for n, _ in c.kernel_timeline(64)]


def n_cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def current_groups(T, n_pairs, S):
    """k_species_current's group count (species_sum.hip: species_sum_parts; 4, 2, 1 frames per thread for S <= 2, 4, 8)."""
    rows = 4 if S <= 2 else 2 if S <= 4 else 1
    n_tb = -(-T // (256 * rows))
    return max(1, min(-(-8 * n_cu() // n_tb), n_pairs, 1024))


def run_staged(c, fft, lab, w, S):
    """ta_current_staged into caller buffers, twice: the two runs must agree bit for bit."""
    import torch

    dev = torch.device("cuda", 0)
    T, _, D = c.shape
    d_lab = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).to(dev)
    d_w = torch.from_numpy(np.ascontiguousarray(w)).to(dev) if w is not None else None
    runs = []
    for _ in range(2):
        cur = torch.full((S, T, D), np.nan, dtype=torch.float64, device=dev)
        cr = torch.full((T, S, S), np.nan, dtype=torch.float64, device=dev)
        c.current_staged(fft, S, d_lab.data_ptr(), cur.data_ptr(), d_w.data_ptr() if d_w is not None else 0, cr.data_ptr())
        torch.cuda.synchronize()
        runs.append((cur.cpu().numpy(), cr.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "repeat runs differ"
    return runs[0]


def slab_padding(c, dtype):
    """(rows T ... pitch - 1 of every pair, the phantom column's rows or None) of the raw device slab"""
    T, A, D = c.shape
    ptr, pitch, n_pairs = c.stage_device(0)
    raw = np.empty(n_pairs * pitch * 2, dtype=dtype)
    L = _lib.lib()
    L.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert L.hipMemcpy(raw.ctypes.data, ptr, raw.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    raw = raw.reshape(n_pairs, pitch, 2)
    return raw[:, T:, :], (raw[-1, :, 1] if (A * D) % 2 else None)


# (id, T, A, D, S, labels): "alt" = species n % S atom by atom, so that with D = 3 every straddling pair holds two
# species; "rand" = current_ref's random order with unequal sizes
SHAPE_CASES = [
    ("straddle_odd_cols_d3", 1100, 1501, 3, 2, "alt"),
    ("straddle_d3_s3", 1101, 1501, 3, 3, "alt"),
    ("d2", 2049, 1100, 2, 4, "alt"),
    ("odd_cols_d1", 2048, 2101, 1, 5, "alt"),
    ("s1", 1100, 1501, 3, 1, "rand"),
    ("s8", 1101, 1501, 3, 8, "rand"),
    ("long_outer_radix", 20000, 211, 3, 2, "rand"),
    ("t1", 1, 700, 3, 3, "rand"),
    ("t2", 2, 700, 3, 4, "rand"),
    ("t3", 3, 700, 3, 8, "rand"),
    ("t1023", 1023, 700, 3, 2, "rand"),
    ("t1024", 1024, 700, 3, 4, "rand"),
    ("t1025", 1025, 700, 3, 8, "rand"),
    ("t2049_s5", 2049, 700, 3, 5, "rand"),
]


@functools.lru_cache(maxsize=4)
def shape_case(T, A, D, S, labels):
    v, lab, w = species_velocities(T, A, S, seed=T + A + S + D, D=D)
    v = v.astype(np.float32).astype(np.float64)  # the same values in both slab types
    if labels == "alt":
        lab = (np.arange(A) % S).astype(np.int32)
    J, scale = currents_ref(v, lab, w, S)
    return v, lab, w, J, scale, cross_ref(J)


def cross_kernels(T, fft):
    """a kernel only the correlator of this length and fft launches (api.hip: fft_impl / direct_impl)"""
    if T <= 64:
        return {"k_short"}
    if fft:
        return {"k_w1_bp"} if T <= 512 else {"k_wsplit_accum", "k_winverse"}
    return set()  # the direct forms by their own thresholds: named by the VACF tests


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("T,A,D,S,labels", [pytest.param(*c[1:], id=f"{c[0]}-T{c[1]}-A{c[2]}-D{c[3]}-S{c[4]}") for c in SHAPE_CASES])
def test_species_current_shapes(T, A, D, S, labels, dtype):
    v, lab, w, want_j, scale, want_c = shape_case(T, A, D, S, labels)
    n_pairs = (A * D + 1) // 2
    assert n_pairs > current_groups(T, n_pairs, S), "each k_species_current group must take several pairs"
    c = staged_context(v, dtype)
    try:
        for fft in (True, False):
            j, cr = run_staged(c, fft, lab, w, S)
            names = timeline(c)
            assert "k_species_current" in names, names
            assert "k_widen_f32" not in names, names  # the slab is read in its own element type
            assert {"k_onsager_combos", "k_current_finish"} | cross_kernels(T, fft) <= set(names), names
            assert_currents(j, want_j, scale)
            assert_cross(cr, want_c)
        j2, none = c.current(True, lab, n_species=S, weights=w, cross=False)  # the host-facing call, the currents alone
        assert none is None and np.array_equal(j2, j)
        tail, phantom = slab_padding(c, dtype)
        assert not tail.any(), "rows T ... pitch - 1 of the slab must still be zero"
        assert phantom is None or not phantom.any(), "the phantom column must still be zero"
    finally:
        c.close()


@pytest.mark.parametrize("dtype", SLABS)
def test_current_dev_wide_rows(dtype):
    """ta_current_dev on a frame-major float64 tensor with ld_row > n_atoms * dim equals the staged path bit for bit
    (the staged slab in either element type: the values are float32-representable and every sum is formed in float64
    in the same order)."""
    import torch

    T, A, D, S = 1101, 301, 3, 3
    ld_row = A * D + 7
    v, lab, w, want_j, scale, want_c = shape_case(T, A, D, S, "rand")
    wide = np.full((T, ld_row), 7.5e3)
    wide[:, :A * D] = v.reshape(T, A * D)
    dev = torch.device("cuda", 0)
    d_v, d_lab, d_w = torch.from_numpy(wide).to(dev), torch.from_numpy(np.array(lab)).to(dev), torch.from_numpy(np.array(w)).to(dev)
    c = staged_context(v, dtype)
    try:
        for fft in (True, False):
            j, cr = run_staged(c, fft, lab, w, S)
            cur = torch.zeros((S, T, D), dtype=torch.float64, device=dev)
            cross = torch.zeros((T, S, S), dtype=torch.float64, device=dev)
            c.current_dev(d_v.data_ptr(), T, A, D, ld_row, fft, S, d_lab.data_ptr(), cur.data_ptr(), d_w.data_ptr(),
                          cross.data_ptr())
            torch.cuda.synchronize()
            names = timeline(c)
            assert "k_relayout" in names and "k_species_current" in names and "k_widen_f32" not in names, names
            assert np.array_equal(cur.cpu().numpy(), j) and np.array_equal(cross.cpu().numpy(), cr)
            assert_currents(j, want_j, scale)
            assert_cross(cr, want_c)
    finally:
        c.close()
