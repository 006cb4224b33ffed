"""oracle/exact.py without a GPU: the exact numerators against Python integers, the correctly rounded expectations
against the NumPy oracle, the guards and the budget on inputs that break them, the np.longdouble reference against
rational arithmetic, and the FFT error model of test_exact_parity.py checked on this host -- NumPy's FFT and the
library's CPU backend meet the bound [C u log2(L) E + 4 u S1(k)] / (T - k) with the same C, before any GPU runs."""
import math

import numpy as np
import pytest

from oracle import exact as ex
from oracle import numpy_oracle as orc
from transport_analysis_amd import _lib


def brute_corr(a):
    T, n = a.shape
    ai = [[int(t) for t in row] for row in a]
    return [[sum(ai[i][c] * ai[i + k][c] for i in range(T - k)) for c in range(n)] for k in range(T)]


def brute_sqdiff(a):
    T, n = a.shape
    ai = [[int(t) for t in row] for row in a]
    return [[sum((ai[i][c] - ai[i + k][c]) ** 2 for i in range(T - k)) for c in range(n)] for k in range(T)]


@pytest.mark.parametrize("T,n", [(1, 1), (2, 3), (7, 2), (64, 3), (65, 2), (130, 3)])
def test_numerators_match_python_integers(T, n):
    a = np.random.default_rng(T + n).integers(-3000, 3001, size=(T, n)).astype(np.float64)
    assert ex.correlate_cols(a).tolist() == brute_corr(a)
    assert ex.sqdiff_cols(a).tolist() == brute_sqdiff(a)
    assert ex.sqdiff_cols(a)[0].tolist() == [0] * n


def test_fft_numerators_equal_np_correlate():
    a = ex.int_walk(3000, 4, 2, 5, seed=1, drift=1).reshape(3000, 8)
    a = a - a[0]
    assert np.array_equal(ex.correlate_cols(a, sample=8), ex.correlate_cols(a, fft_from=10 ** 9))


def test_fft_numerators_guard_rejects_what_rint_cannot_recover():
    # |a| ~ 2^22 over 4096 frames: C ~ 2^56, beyond exact float64 integers, so the FFT lies far from any integer
    a = np.random.default_rng(2).integers(-2 ** 22, 2 ** 22, size=(4096, 2)).astype(np.float64)
    with pytest.raises(AssertionError, match="integer"):
        ex.correlate_cols(a)
    with pytest.raises(ValueError):
        ex.correlate_cols(a + 0.5)


def test_budget_accepts_and_rejects():
    a = np.full((10, 3), 1000.0)
    assert ex.budget(a, 30) == 1000
    with pytest.raises(AssertionError, match="integer"):
        ex.budget(a + 0.25, 30)
    with pytest.raises(AssertionError, match="2\\^53"):
        ex.budget(np.array([2.0 ** 25]), 10 ** 4)  # 1e4 (2^26)^2 > 2^53
    # float32: F32_TERMS (2 max|a|)^2 < 2^24 admits |a| <= 18
    assert ex.budget(np.array([-18.0, 3.0]), 100, f32=True) == 18
    with pytest.raises(AssertionError, match="2\\^24"):
        ex.budget(np.array([19.0]), 100, f32=True)


def test_divide_is_correctly_rounded_and_ulps():
    num = np.array([1, 2, 10 ** 17 + 1, -(2 ** 60) - 3], dtype=np.int64)
    den = np.array([3, 7, 3, 5], dtype=np.int64)
    got = ex.divide(num, den)
    from fractions import Fraction

    for g, n, d in zip(got, num, den):
        assert g == float(Fraction(int(n), int(d)))
    assert ex.ulps(1.0, 1.0) == 0 and ex.ulps(np.nextafter(1.0, 2.0), 1.0) == 1
    assert ex.ulps(1e-300, 0.0) == np.inf and ex.ulps(0.0, 0.0) == 0


@pytest.mark.parametrize("T,A", [(1, 3), (2, 4), (90, 5), (700, 3)])
def test_exact_expectations_match_the_numpy_oracle(T, A):
    """Within 2 ulps at every lag and particle.  Helfand at D = 2 (the /D is exact there, so the oracle's mean over D
    and then over time rounds once)."""
    v = ex.int_velocities(T, A, 3, 50, seed=3)
    x = ex.int_walk(T, A, 3, 4, seed=4, offset=2 ** 30)
    m = ex.int_masses(A, 1, 20, seed=5)
    q = ex.int_charges(A, 3, seed=6)
    den = ex.lag_den(T)[:, None]
    want = ex.divide(ex.vacf_num(v), den)
    assert ex.ulps(orc.vacf_windowed(v)[0], want).max() <= 2
    v2, x2 = v[:, :, :2], x[:, :, :2] - 2 ** 30
    want = ex.divide(ex.helfand_num(v2, x2, m), 2 * den)
    got = orc.helfand(v2, x2, m, np.ones(T), 1.0, boltzmann=0.5)[0]  # scale 1 / (2 kB V T) = 1
    assert ex.ulps(got, want).max() <= 2
    want = ex.divide(ex.msd_num(x), den)
    assert ex.ulps(orc.msd_at_lags(x, np.arange(T)), want).max() <= 2
    M = ex.moment_exact(x, q)
    assert np.array_equal(orc.cond_moment(x, q)[0], M.astype(np.float64))
    assert ex.ulps(orc.moment_msd(M), ex.divide(ex.phi_num(M), ex.lag_den(T))).max() <= 2
    assert ex.ulps(orc.self_term_at_lags(x, q, np.arange(T)), ex.divide(ex.self_num(x, q), ex.lag_den(T))).max() <= 2


@pytest.mark.parametrize("shift", [True, False], ids=["moments", "currents"])
def test_species_sums_and_pseudo_particle_numerators_match_fractions(shift):
    """Three species (one of a single atom), seven frames: species_moment_exact against sums of Fractions atom by atom,
    pseudo_particles in slab order, pseudo_num against the lag sums of each pseudo-particle in rational arithmetic, and
    the polarisation identity 1/4 (R+ - R-) = the cross term of Q_i and Q_j."""
    from fractions import Fraction

    T, A, D, S = 7, 6, 2, 3
    y = ex.int_walk(T, A, D, 4, seed=11, offset=2 ** 30) if shift else ex.int_velocities(T, A, D, 50, seed=11)
    q = ex.int_charges(A, 3, seed=12)
    lab = np.array([0, 2, 0, 1, 2, 0])
    Q = ex.species_moment_exact(y, q, lab, S, shift=shift)
    assert Q.shape == (S, T, D) and Q.dtype == np.int64
    for s in range(S):
        for t in range(T):
            for d in range(D):
                want = sum(Fraction(q[n]) * (Fraction(y[t, n, d]) - (Fraction(y[0, n, d]) if shift else 0))
                           for n in range(A) if lab[n] == s)
                assert Q[s, t, d] == want
    assert not ex.species_moment_exact(y, q, lab, 4, shift=shift)[3].any()  # a label nobody carries
    P = ex.pseudo_particles(Q)
    assert P.shape == (T, S * S, D)
    for i in range(S):
        for j in range(S):
            assert np.array_equal(P[:, i * S + j], Q[i] if i == j else Q[i] + Q[j] if i < j else Q[i] - Q[j])
    R = ex.pseudo_num(Q, acf=not shift)
    assert np.array_equal(R, ex.pseudo_num(Q, acf=not shift, fft_from=4))  # (7 frames: int64 products either way)
    for p in range(S * S):
        for k in range(T):
            f = (ex.frac_sqdiff if shift else ex.frac_corr)
            assert R[k, p] == sum(f(P[:, p, d].astype(np.float64), k) for d in range(D))
    for i in range(S):
        for j in range(i + 1, S):
            for k in range(T):
                if shift:
                    cross = sum(int((Q[i, t + k, d] - Q[i, t, d]) * (Q[j, t + k, d] - Q[j, t, d]))
                                for t in range(T - k) for d in range(D))
                    assert R[k, i * S + j] + R[k, j * S + i] == 2 * (R[k, i * S + i] + R[k, j * S + j])
                else:
                    cross = Fraction(sum(int(Q[i, t, d] * Q[j, t + k, d] + Q[j, t, d] * Q[i, t + k, d])
                                         for t in range(T - k) for d in range(D)), 2)
                assert Fraction(int(R[k, i * S + j] - R[k, j * S + i]), 4) == cross


needs_longdouble = pytest.mark.skipif(not ex.longdouble_ok(), reason="np.longdouble has no 64-bit significand here")


@needs_longdouble
def test_longdouble_reference_against_fractions():
    rng = np.random.default_rng(7)
    a = 1e4 + np.cumsum(rng.standard_normal((300, 2)), axis=0)
    lags = [1, 2, 17, 150, 299]
    c, s = ex.ld_corr(a, lags), ex.ld_sqdiff(a, lags)
    for j, k in enumerate(lags):
        for col in range(2):
            fc, fs = ex.frac_corr(a[:, col], k), ex.frac_sqdiff(a[:, col], k)
            assert abs(ex.to_fraction(c[j, col]) - fc) <= 2.0 ** -58 * fc
            assert abs(ex.to_fraction(s[j, col]) - fs) <= 2.0 ** -58 * fs


def test_fft_energy_pairs_particles():
    e = np.array([1.0, 2.0, 4.0, 8.0, 16.0])
    assert ex.fft_energy_bp(e).tolist() == [3.0, 3.0, 12.0, 12.0, 16.0]


def hetero_velocities(T, A, D, seed):
    """Standard normal velocities, particle n scaled by 2^s_n with s_n cycling 0, -12, -24, -36."""
    s = np.array([(0, -12, -24, -36)[n % 4] for n in range(A)])
    return orc.synthetic_velocities(T, A, D, seed=seed) * np.ldexp(1.0, s)[None, :, None]


def fft_ratios(bp, ts, v, L, msd=False):
    """Worst |err| / bound over the lag sample: by particle and for the lag sums (a mean over particles)."""
    T, A, D = v.shape
    lags = orc.lag_sample(T)
    a = v - v[0] if msd else v
    ref_cols = (ex.ld_sqdiff if msd else ex.ld_corr)(v.reshape(T, A * D), lags).reshape(len(lags), A, D).sum(axis=2)
    den = (T - lags).astype(np.longdouble)[:, None]
    ref = ref_cols / den
    e = ex.column_energy(a).sum(axis=1)
    S1 = ex.s1_float(a).sum(axis=2) if msd else None
    bound = ex.fft_bound(T, L, ex.fft_energy_bp(e), S1)[lags]
    r_bp = (np.abs(bp[lags] - ref) / bound).astype(np.float64)
    r_bp[bound == 0] = 0.0
    b_ts = ex.fft_bound(T, L, e.sum(), S1.sum(axis=1) if msd else None)[lags] / A
    r_ts = (np.abs(ts[lags] - ref.sum(axis=1) / A) / b_ts).astype(np.float64)
    return float(r_bp.max()), float(r_ts.max())


@needs_longdouble
@pytest.mark.parametrize("T,A,D", [(30, 5, 3), (100, 6, 2), (257, 7, 1), (1000, 5, 3), (3500, 4, 3), (10300, 3, 2)])
def test_fft_error_model_on_the_host(T, A, D):
    """NumPy's FFT (tidynamics' padding) and the CPU backend's radix-4 FFT within the bound of test_exact_parity.py,
    by particle (E over the particle pair that shares a transform) and for the lag sums, VACF and MSD."""
    v = hetero_velocities(T, A, D, seed=T)
    bp, ts = orc.vacf_fft_batched(v)
    L_np = 2 * orc.tidynamics_n_fft(T)
    r_bp, r_ts = fft_ratios(bp, ts, v, L_np)
    assert r_bp <= 1.0 and r_ts <= 1.0, ("numpy", r_bp, r_ts)
    c = _lib.Context("cpu")
    try:
        (slab,) = c.stage_alloc(T, A, D)
        slab[:] = v
        c.stage_commit(0, T)
        ts_c, bp_c = c.vacf_fft(by_particle=True)
        L_cpu = 1 << int(math.ceil(math.log2(2 * T)))
        r_bp, r_ts = fft_ratios(bp_c, ts_c, v, L_cpu)
        assert r_bp <= 1.0 and r_ts <= 1.0, ("cpu backend vacf", r_bp, r_ts)
        x = 1e4 + np.cumsum(v, axis=0) + 0.3 * np.arange(T)[:, None, None]
        slab[:] = x
        c.stage_commit(0, T)
        ts_m, bp_m = c.msd(True, by_particle=True)
        r_bp, r_ts = fft_ratios(bp_m, ts_m, x, L_cpu, msd=True)
        assert r_bp <= 1.0 and r_ts <= 1.0, ("cpu backend msd", r_bp, r_ts)
    finally:
        c.close()
