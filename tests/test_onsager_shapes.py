"""k_species_moment and the cross MSD at shapes that reach every branch of the kernel, through the C-ABI (the staged and
the frame-major device entry points), GPU only.  Every case asserts k_species_moment in the kernel timeline and compares
the moments at every frame, and C at every lag and for all S^2 pairs, with the long-double references of onsager_ref:

  * column pairs that straddle two atoms OF DIFFERENT SPECIES (D = 3, labels alternating atom by atom), odd column counts
    (the unpaired last column), D = 2 and D = 1;
  * every species class of the kernel template and both ends of each: S = 1, 2 | 3, 4 | 5, 8;
  * more column pairs than groups of pairs, so one group sums pairs of several species; 20000 frames (20 frame blocks,
    few groups, an outer-radix FFT plan for C); 1, 2 and 1023 ... 1025 frames (partial frame blocks);
  * two nearly neutral species sharing a drift (the shift comes before the weight);
  * frame-major input with ld_row > n_atoms dim; a float32 device slab."""
import functools

import numpy as np
import pytest

from onsager_ref import assert_cross, assert_moments, cross_ref, moments_ref, species_walk, walk_case
from transport_analysis_amd import _lib

pytestmark = pytest.mark.gpu


def staged_context(x, dtype=np.float64, device_f32=False):
    T, A, D = x.shape
    c = _lib.Context(0)
    if device_f32:
        c.set_option("stage_device_f32", 1)
    (view,) = c.stage_alloc(T, A, D, dtype=dtype)
    view[:] = x
    c.stage_commit(0, T)
    c.set_option("timeline", 1)
    return c


def timeline(c):
    return [n for n, _ in c.kernel_timeline(64)]


def n_cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def moment_groups(T, n_pairs, S):
    """k_species_moment's group count (species_sum.hip: species_sum_parts; 4, 2, 1 rows per thread for S <= 2, 4, 8)."""
    rows = 4 if S <= 2 else 2 if S <= 4 else 1
    n_tb = -(-T // (256 * rows))
    return max(1, min(-(-8 * n_cu() // n_tb), n_pairs, 1024))


def cross_kernel(T, fft):
    return "k_short" if T <= 64 else "k_msd_prepare" if fft else "k_mid" if T <= 512 else "k_direct"


def run_staged(c, fft, lab, w, S):
    """ta_onsager_staged into caller buffers, twice: the two runs must agree bit for bit."""
    import torch

    dev = torch.device("cuda", 0)
    T, _, D = c.shape
    d_lab = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).to(dev)
    d_w = torch.from_numpy(np.ascontiguousarray(w)).to(dev) if w is not None else None
    runs = []
    for _ in range(2):
        mom = torch.full((S, T, D), np.nan, dtype=torch.float64, device=dev)
        cr = torch.full((T, S, S), np.nan, dtype=torch.float64, device=dev)
        c.onsager_staged(fft, S, d_lab.data_ptr(), mom.data_ptr(), d_w.data_ptr() if d_w is not None else 0, cr.data_ptr())
        torch.cuda.synchronize()
        runs.append((mom.cpu().numpy(), cr.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "repeat runs differ"
    return runs[0]


# (id, T, A, D, S, labels): "alt" = species n % S atom by atom, so that with D = 3 every straddling pair holds two
# species; "walk" = onsager_ref's random order with unequal sizes
SHAPE_CASES = [
    ("straddle_odd_cols_d3", 1100, 1501, 3, 2, "alt"),
    ("straddle_d3_s3", 1100, 1501, 3, 3, "alt"),
    ("d2", 2049, 1100, 2, 4, "alt"),
    ("odd_cols_d1", 2048, 2101, 1, 5, "alt"),
    ("s1", 1100, 1501, 3, 1, "walk"),
    ("s8", 1100, 1501, 3, 8, "walk"),
    ("long_outer_radix", 20000, 211, 3, 2, "walk"),
    ("t1", 1, 700, 3, 3, "walk"),
    ("t2", 2, 700, 3, 4, "walk"),
    ("t1023", 1023, 700, 3, 2, "walk"),
    ("t1024", 1024, 700, 3, 4, "walk"),
    ("t1025", 1025, 700, 3, 8, "walk"),
]


@functools.lru_cache(maxsize=4)
def shape_case(T, A, D, S, labels):
    if labels == "walk":
        return walk_case(T, A, S, D=D)
    x, _, w = species_walk(T, A, S, seed=T + A + S + D, D=D)
    lab = (np.arange(A) % S).astype(np.int32)
    M, scale = moments_ref(x, lab, w, S)
    return x, lab, w, M, scale, cross_ref(M)


@pytest.mark.parametrize("T,A,D,S,labels", [pytest.param(*c[1:], id=f"{c[0]}-T{c[1]}-A{c[2]}-D{c[3]}-S{c[4]}") for c in SHAPE_CASES])
def test_species_moment_shapes(T, A, D, S, labels):
    x, lab, w, want_m, scale, want_c = shape_case(T, A, D, S, labels)
    n_pairs = (A * D + 1) // 2
    groups = moment_groups(T, n_pairs, S)
    assert n_pairs > groups, "each k_species_moment group must take several pairs"
    c = staged_context(x)
    try:
        for fft in (True, False):
            m, cr = run_staged(c, fft, lab, w, S)
            names = timeline(c)
            assert "k_species_moment" in names, names
            if T >= 2:  # (one frame: lag 0 alone, nothing to correlate)
                assert {"k_onsager_combos", cross_kernel(T, fft), "k_onsager_finish"} <= set(names), names
            assert_moments(m, want_m, scale)
            assert_cross(cr, want_c)
        m2, none = c.onsager(True, lab, n_species=S, weights=w, cross=False)  # the host-facing call, the moments alone
        assert none is None and np.array_equal(m2, m)
    finally:
        c.close()


def test_near_neutral_species_with_shared_drift():
    """Two species whose weights nearly cancel inside each species, on walks that share a drift of ~30 steps per step:
    the moments are far below sum |w| |dx|, which only holds up if the first frame is subtracted before the weight."""
    T, A, S = 1100, 1501, 2
    x, lab, _ = species_walk(T, A, S, seed=77, drift=30.0)
    rng = np.random.default_rng(78)
    w = rng.uniform(-1.5, 1.5, size=A)
    for s in range(S):
        w[lab == s] -= w[lab == s].mean()
    w[0] += 1e-6  # not exactly neutral
    want_m, scale = moments_ref(x, lab, w, S)
    assert (np.abs(want_m).max(axis=(1, 2)) < 0.05 * scale).all()  # the drift cancels
    c = staged_context(x)
    try:
        for fft in (True, False):
            m, cr = run_staged(c, fft, lab, w, S)
            assert "k_species_moment" in timeline(c)
            assert_moments(m, want_m, scale)
            assert_cross(cr, cross_ref(want_m))
    finally:
        c.close()


def test_onsager_dev_wide_rows():
    """ta_onsager_dev on a frame-major tensor with ld_row > n_atoms * dim equals the staged path bit for bit."""
    import torch

    T, A, D, S = 1100, 301, 3, 3
    ld_row = A * D + 7
    x, lab, w, want_m, scale, want_c = walk_case(T, A, S)
    wide = np.full((T, ld_row), 7.5e3)
    wide[:, :A * D] = x.reshape(T, A * D)
    dev = torch.device("cuda", 0)
    d_x, d_lab, d_w = torch.from_numpy(wide).to(dev), torch.from_numpy(np.array(lab)).to(dev), torch.from_numpy(np.array(w)).to(dev)
    c = staged_context(x)
    try:
        for fft in (True, False):
            m, cr = run_staged(c, fft, lab, w, S)
            mom = torch.zeros((S, T, D), dtype=torch.float64, device=dev)
            cross = torch.zeros((T, S, S), dtype=torch.float64, device=dev)
            c.onsager_dev(d_x.data_ptr(), T, A, D, ld_row, fft, S, d_lab.data_ptr(), mom.data_ptr(), d_w.data_ptr(),
                          cross.data_ptr())
            torch.cuda.synchronize()
            names = timeline(c)
            assert "k_relayout" in names and "k_species_moment" in names, names
            assert np.array_equal(mom.cpu().numpy(), m) and np.array_equal(cross.cpu().numpy(), cr)
            assert_moments(m, want_m, scale)
            assert_cross(cr, want_c)
    finally:
        c.close()


def test_float32_device_slab():
    """A float32-staged slab kept as float32 on the device ("stage_device_f32"): widened first, then the same pass."""
    T, A, S = 1100, 301, 4
    x, lab, w, want_m, scale, want_c = walk_case(T, A, S, f32=True)
    c = staged_context(x, dtype=np.float32, device_f32=True)
    try:
        for fft in (True, False):
            m, cr = run_staged(c, fft, lab, w, S)
            names = timeline(c)
            assert "k_widen_f32" in names and "k_species_moment" in names, names
            assert_moments(m, want_m, scale)
            assert_cross(cr, want_c)
    finally:
        c.close()
