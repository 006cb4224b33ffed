"""The forward kernel of the two largest on-chip plans (R0 = 18: 8193 ... 9216 frames, R0 = 20: 9217 ... 10240), whose
lag-sum variants carry one specialised first stage per pass (wfft.hpp, wf_accum_body<..., PASS>): pass 0 without `h`,
pass 1 with the twist inside the butterfly, the output-twiddle seeds squared from one table read.  Lag sums only, on
float64 slabs and on float32 device slabs ("stage_device_f32"; the oracle then sees the input rounded to float32), at
the smallest and largest lengths of either plan -- twist, seeds and the zero-padded rows 10000 ... 10239 differ between
them -- against oracle.numpy_oracle.vacf_fft_batched, scale-relative 1e-10.

  * (A, D) = (1, 3): two column pairs, the second half empty; nearly every tuple has no unit (the zero-row path);
  * (A, D) = (90, 3): 135 pairs against 128 tuples on 256 compute units, some tuples run two units and some one
    (the loop-carried state);
  * (A, D) = (7, 1): an odd column count.
"""
import numpy as np
import pytest

from conftest import scale_rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-10
FRAMES = [9217, 10000, 10240, 8193, 9216]  # R0 = 20 (three), R0 = 18 (two)
ATOMS = [(1, 3), (90, 3), (7, 1)]
SLABS = [pytest.param(np.float64, id="slab64"), pytest.param(np.float32, id="slab32")]


@pytest.fixture(scope="module")
def ctx():
    from transport_analysis_amd import _lib

    assert _lib.device_count() >= 1, "no GPU visible: the HIP path cannot run"
    c = _lib.Context(0)
    yield c
    c.close()


def stage(c, v, dtype):
    T, A, D = v.shape
    c.set_option("stage_device_f32", int(dtype == np.float32))
    (slab,) = c.stage_alloc(T, A, D, dtype=dtype)
    slab[...] = v
    c.stage_commit(0, T)


@pytest.mark.parametrize("dtype", SLABS)
@pytest.mark.parametrize("A,D", ATOMS)
@pytest.mark.parametrize("T", FRAMES)
def test_forward_pass_split_vs_oracle(ctx, T, A, D, dtype):
    from oracle import numpy_oracle as orc

    v = orc.synthetic_velocities(T, A, D, seed=1000 + T).astype(dtype)
    _, want_ts = orc.vacf_fft_batched(v.astype(np.float64))
    stage(ctx, v, dtype)
    ts, bp = ctx.vacf_fft(by_particle=False)
    assert bp is None
    err = scale_rel_err(ts, want_ts)
    print(f"T={T} A={A} D={D} {np.dtype(dtype).name}: scale-relative error {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("dtype", SLABS)
def test_forward_pass_split_repeats_bit_equal(ctx, dtype):
    from oracle import numpy_oracle as orc

    stage(ctx, orc.synthetic_velocities(10000, 90, 3, seed=11000).astype(dtype), dtype)
    first, _ = ctx.vacf_fft(by_particle=False)
    second, _ = ctx.vacf_fft(by_particle=False)
    assert np.array_equal(np.asarray(first), np.asarray(second))
