"""ShellResidence on the GPU (device=0) against the CPU backend (device="cpu") and against shell_ref, on both stage dtypes:
with fft=False every result is equal, with fft=True the counts and the survival function are equal and the intermittent
function is within the FFT path's 1e-10 of ci[0]."""
import numpy as np
import pytest

import shell_ref as ref
from test_pair_lifetime import DIM_TYPES
from test_shell_residence import class_against_reference, universe
from transport_analysis_amd import ShellResidence

pytestmark = pytest.mark.gpu

KEYS = ("times", "n_inside", "mean_inside", "run_lengths", "survival", "intermittent", "tau_residence", "tau_intermittent", "mean_run")


@pytest.mark.parametrize("stage_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_class_gpu_equals_cpu_and_reference(D, stage_dtype):
    for kind, boxed, gap in (("disjoint", False, 0), ("disjoint", True, 2), ("same", "frames", 1)):
        g = class_against_reference(kind, D, boxed, gap, device=0, stage_dtype=stage_dtype)
        x, a, b, dims, axes, cuts, s, _ = ref.case(40, 6, 30, D, kind, boxed, gap)
        u = universe(x, dims, axes)
        groups = (u.atoms,) if kind == "same" else (u.atoms[a], u.atoms[b])
        h = ShellResidence(*groups, r_cut=cuts["r_cut"], r_break=cuts["r_break"], intermittency=gap, periodic=dims is not None,
                           fft=False, dim_type=DIM_TYPES[D], device="cpu", stage_dtype=stage_dtype).run().results
        for key in KEYS:
            assert np.array_equal(np.asarray(getattr(g, key)), np.asarray(getattr(h, key)), equal_nan=True), key


def test_class_larger_than_a_tile():
    """1100 observed atoms (two b-tiles) around 20 reference atoms in a box, 70 frames, float32 staging: the class on the GPU
    equals the reference's integers and the CPU backend's results"""
    x, a, b, dims, axes, cuts, s, (ci, runs, nb, cc) = ref.case(70, 20, 1100, 3, "disjoint", True, 1)
    u = universe(x, dims, axes)
    kw = dict(r_cut=cuts["r_cut"], r_break=cuts["r_break"], intermittency=1, fft=False, stage_dtype=np.float32)
    g = ShellResidence(u.atoms[a], u.atoms[b], device=0, **kw).run().results
    h = ShellResidence(u.atoms[a], u.atoms[b], device="cpu", **kw).run().results
    assert np.array_equal(g.n_inside, nb) and np.array_equal(g.run_lengths, runs)
    for key in KEYS:
        assert np.array_equal(np.asarray(getattr(g, key)), np.asarray(getattr(h, key)), equal_nan=True), key
