"""ShellMSD on the GPU (device=0) against the CPU backend (device="cpu") and against shell_msd_ref, on both stage dtypes and
under both conditions: every result key is equal (the inputs are on the grid: every sum is exact)."""
import numpy as np
import pytest

import shell_msd_ref as mref
from test_shell_msd import class_results
from transport_analysis_amd import ShellMSD
from transport_analysis_amd._mini_mda import ArrayUniverse

pytestmark = pytest.mark.gpu

KEYS = ("times", "count", "msd_axes", "msd", "n_inside", "mean_inside", "run_lengths", "survival")


@pytest.mark.parametrize("stage_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_class_gpu_equals_cpu_and_reference(D, stage_dtype):
    for condition in mref.CONDITIONS:
        for kind, boxed, gap, L in (("disjoint", False, 0, 39), ("disjoint", True, 2, 20), ("same", "frames", 1, 25)):
            g = class_results(kind, D, boxed, gap, L, condition, device=0, stage_dtype=stage_dtype)
            h = class_results(kind, D, boxed, gap, L, condition, device="cpu", stage_dtype=stage_dtype)
            for key in KEYS:
                assert np.array_equal(np.asarray(getattr(g, key)), np.asarray(getattr(h, key)), equal_nan=True), key


@pytest.mark.parametrize("stage_dtype", [np.float64, np.float32])
def test_class_larger_than_a_tile_unwrapped(stage_dtype):
    """1100 observed atoms (two b-tiles) around 20 reference atoms, 70 frames, wrapped into the box and unwrap=True: the class
    on the GPU equals the reference's integers on the walk itself and the CPU backend's results"""
    L = 50
    x, a, b, dims, axes, cuts, g, want, runs, nb = mref.case(70, 20, 1100, 3, "disjoint", True, 1, L)
    box = dims[:, :3]
    xw = x - np.floor(x / box[:, None, :]) * box[:, None, :]
    assert np.array_equal(mref.nojump(xw, box) - xw[0], x - x[0])
    u = ArrayUniverse(positions=xw, dimensions=dims)
    kw = dict(r_cut=cuts["r_cut"], r_break=cuts["r_break"], intermittency=1, max_lag=L, unwrap=True, stage_dtype=stage_dtype)
    for condition in mref.CONDITIONS:
        S, N = want[condition]
        r = ShellMSD(u.atoms[a], u.atoms[b], device=0, condition=condition, **kw).run().results
        h = ShellMSD(u.atoms[a], u.atoms[b], device="cpu", condition=condition, **kw).run().results
        assert np.array_equal(r.count, N) and np.array_equal(r.n_inside, nb) and np.array_equal(r.run_lengths, runs)
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.array_equal(r.msd_axes, np.where(N[:, None] > 0, S / N[:, None], np.nan), equal_nan=True)
        for key in KEYS:
            assert np.array_equal(np.asarray(getattr(r, key)), np.asarray(getattr(h, key)), equal_nan=True), key
