"""The split forward bodies (R0 = 18, 20, lag sums, float64 slab; wfft.hpp, kAlongC) request the next unit's rows
behind the last-stage butterflies of S2, a group into the registers of each sub-series as it retires, instead of in one burst
behind S2.  A row that lands in a register still in use, a group left out on one of the two paths (three sub-series at a time,
two at a time), or a prefetch that runs on after the tuple's last unit shows in the lag sums: every lag of ta_vacf_fft_staged is
compared with oracle.numpy_oracle.vacf_fft_batched, scale-relative 1e-10 (the project's parity bar).

  * frames 8705 / 9216 (R0 = 18: shortest, exact), 9217 / 10000 / 10240 (R0 = 20: shortest, padded inside M, exact);
  * (A, 3) on 128 tuples per pass (one tuple is one pair of workgroups): A = 1 (two column pairs: most tuples have no unit
    and store the zero row, the others' first prefetch is already past the end), 90 (135 pairs: tuples with one and with two
    units, the last prefetch reads the empty buffer) and 171 (257 pairs: two and three units);
  * 10240 and then 8705 frames on the same context, twice each: the second plan's launch follows the first one's on the same
    buffers, and a repeated call gives the same bits;
  * beyond 10240 frames the same two plans run behind an outer radix R, their rows requested the same way: 18000 frames
    (R0 = 18, R = 2), 20000 (R0 = 20, R = 2) and 30000 (R0 = 20, R = 3) at (45, 3): 68 pairs on 64 / 40 tuples per pass, tuples
    with one and with two units.
"""
import numpy as np
import pytest

from conftest import scale_rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-10
FRAMES = [8705, 9216, 9217, 10000, 10240]
ATOMS = [1, 90, 171]


@pytest.fixture(scope="module")
def ctx():
    from transport_analysis_amd import _lib

    assert _lib.device_count() >= 1, "no GPU visible: the HIP path cannot run"
    c = _lib.Context(0)
    c.set_option("stage_device_f32", 0)
    yield c
    c.close()


def lag_sums(c, v):
    T, A, D = v.shape
    (slab,) = c.stage_alloc(T, A, D, dtype=np.float64)
    slab[...] = v
    c.stage_commit(0, T)
    ts, bp = c.vacf_fft(by_particle=False)
    assert bp is None
    return np.array(ts)


@pytest.mark.parametrize("A", ATOMS)
@pytest.mark.parametrize("T", FRAMES)
def test_rows_along_last_stage_vs_oracle(ctx, T, A):
    from oracle import numpy_oracle as orc

    v = orc.synthetic_velocities(T, A, 3, seed=10000 + T + A)
    _, want = orc.vacf_fft_batched(v)
    got = lag_sums(ctx, v)
    assert got.shape == want.shape == (T,)
    err = scale_rel_err(got, want)
    print(f"T={T} A={A}: scale-relative error {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("T", [18000, 20000, 30000])
def test_rows_along_last_stage_outer_radix(ctx, T):
    from oracle import numpy_oracle as orc

    v = orc.synthetic_velocities(T, 45, 3, seed=10700 + T)
    _, want = orc.vacf_fft_batched(v)
    got = lag_sums(ctx, v)
    assert got.shape == want.shape == (T,)
    err = scale_rel_err(got, want)
    print(f"T={T} A=45: scale-relative error {err:.3e}")
    assert err < TOL


def test_rows_along_last_stage_repeated_calls(ctx):
    from oracle import numpy_oracle as orc

    for T in (10240, 8705):
        v = orc.synthetic_velocities(T, 90, 3, seed=10500 + T)
        _, want = orc.vacf_fft_batched(v)
        first = lag_sums(ctx, v)
        second = lag_sums(ctx, v)
        err = scale_rel_err(first, want)
        print(f"T={T}: scale-relative error {err:.3e}, repeated call bit-equal {np.array_equal(first, second)}")
        assert err < TOL
        assert first.tobytes() == second.tobytes()
