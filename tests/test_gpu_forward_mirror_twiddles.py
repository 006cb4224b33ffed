"""The split forward bodies (R0 = 18, 20, lag sums, float64 slab; wfft.hpp, the mirrored output twiddles) generate the first-stage
output twiddles up to R0/2 only and scale the far half of the sub-series by conjugates.  Such a mirrored sub-series has its
512-point transform one bin over, and the accumulators are stored at the address of their true position once per launch.
A bin stored one place off -- or right everywhere except where position (lane >> 3) + 8 (lane & 7) + 64 cc carries from one
digit into the next -- moves energy between lags: every lag of ta_vacf_fft_staged is compared with
oracle.numpy_oracle.vacf_fft_batched, scale-relative 1e-10 (the project's parity bar).

  * frames 8705 / 9216 (R0 = 18: shortest, exact), 9217 / 10000 / 10240 (R0 = 20: shortest, padded inside M, exact);
  * (A, 3) with A = 1 (two column pairs, the second half zeros), 5 (15 columns) and 90 (135 pairs on 128 tuples per pass:
    some tuples run two units, some one; with 2 or 8 pairs most tuples store only the zero row);
  * a concentrated spectrum at (10000, 4, 3): every column a constant plus one cosine whose line sits between two bins of
    a MIRRORED sub-series at a position where the rotation carries (positions 0, 8 b, 64 cc, 511 and their neighbours).
"""
import numpy as np
import pytest

from conftest import scale_rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-10
FRAMES = [8705, 9216, 9217, 10000, 10240]
ATOMS = [1, 5, 90]


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
    return np.asarray(ts)


@pytest.mark.parametrize("A", ATOMS)
@pytest.mark.parametrize("T", FRAMES)
def test_mirror_twiddles_vs_oracle(ctx, T, A):
    from oracle import numpy_oracle as orc

    v = orc.synthetic_velocities(T, A, 3, seed=9000 + T + A)
    _, want = orc.vacf_fft_batched(v)
    got = lag_sums(ctx, v)
    assert got.shape == want.shape == (T,)
    err = scale_rel_err(got, want)
    print(f"T={T} A={A}: scale-relative error {err:.3e}")
    assert err < TOL


def test_mirror_twiddles_concentrated_spectrum(ctx):
    """Bin k = 2 (q + R0 s) + c of the L = 20480 point transform is position s of sub-series q in pass c.  Column j gets
    the period L / (k_j + 1/2), k_j = 2 (q_j + 20 s_j): its line falls between pass 0 and pass 1 of (q_j, s_j), with
    q_j mirrored in both passes (q > 10) and s_j where s -> s - 1 borrows: from lane & 7 (s = 8 b), from cc (s = 64 cc)
    and all the way round (s = 0 <- 511), plus the neighbours that must NOT borrow."""
    from oracle import numpy_oracle as orc

    T, A, D, L, R0 = 10000, 4, 3, 20480, 20
    targets = [(11, 0), (15, 8), (19, 64), (12, 56), (13, 448), (17, 511), (14, 504), (16, 1), (18, 63), (11, 72), (19, 7),
               (15, 449)]
    assert len(targets) == A * D
    t = np.arange(T, dtype=np.float64)
    v = np.empty((T, A, D))
    for j, (q, s) in enumerate(targets):
        period = L / (2 * (q + R0 * s) + 0.5)
        assert (512 / period) % 1 and (L / period) % 1  # divides neither
        v[:, j // D, j % D] = 0.3 + 0.1 * j + (1.0 + 0.25 * j) * np.cos(2 * np.pi * t / period + 0.7 * j)
    _, want = orc.vacf_fft_batched(v)
    got = lag_sums(ctx, v)
    err = np.abs(got - want) / np.max(np.abs(want))
    print(f"concentrated spectrum: scale-relative error {err.max():.3e} (worst lag {int(err.argmax())})")
    assert err.max() < TOL
