"""ShellOrientation on the GPU (device=0) against the CPU backend (device="cpu") and against shell_orient_ref, on both stage
dtypes and under both conditions: every result key is equal (the inputs are on the grid: every sum is exact)."""
import numpy as np
import pytest

import shell_orient_ref as oref
from test_shell_orientation import class_case
from transport_analysis_amd import ShellOrientation

pytestmark = pytest.mark.gpu

KEYS = ("times", "count", "c1", "c2", "n_inside", "mean_inside", "run_lengths", "survival", "tau_1", "tau_2")


@pytest.mark.parametrize("stage_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("mode,anchor,boxed,kind", [("bond", 0, True, "disjoint"), ("bisector", 1, "frames", "disjoint"),
                                                    ("normal", 0, False, "disjoint"), ("bond", 1, "frames", "same")])
def test_class_gpu_equals_cpu_and_reference(mode, anchor, boxed, kind, stage_dtype):
    u, reference, group, vectors, cuts, want, runs, nb = class_case(mode, anchor, boxed, kind)
    kw = dict(mode=mode, anchor=anchor, r_cut=cuts["r_cut"], r_break=cuts["r_break"], intermittency=1, max_lag=30, periodic=bool(boxed),
              stage_dtype=stage_dtype)
    for condition in oref.CONDITIONS:
        g = ShellOrientation(reference, group, vectors, condition=condition, device=0, **kw).run().results
        h = ShellOrientation(reference, group, vectors, condition=condition, device="cpu", **kw).run().results
        S, N = want[condition]
        assert np.array_equal(g.count, N) and np.array_equal(g.n_inside, nb) and np.array_equal(g.run_lengths, runs)
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.array_equal(g.c1, np.where(N > 0, S[:, 0] / N, np.nan), equal_nan=True)
        for key in KEYS:
            assert np.array_equal(np.asarray(getattr(g, key)), np.asarray(getattr(h, key)), equal_nan=True), key
