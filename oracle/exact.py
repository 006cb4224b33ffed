"""Exact and extended-precision references for per-lag, per-particle parity tests.

TEST INFRASTRUCTURE ONLY (see ``oracle/__init__.py``).

The scale-relative bar of the parity tests (``max|got - want| / max|want|``) holds a short lag or a light particle to a
fraction of the LARGEST element.  This module gives every element its own reference:

* Integer-valued inputs.  Every product and every partial sum a direct kernel forms is then an integer; as long as each
  stays below 2^53 (float64 paths) or 2^24 (float32 paths) the kernel's sums are exact in ANY order, and the only
  rounding left is the final scaling.  The numerators are computed exactly here (int64), the expectation is the
  correctly rounded quotient, and a kernel must agree to a few ulps at every lag and every particle.
* Float inputs.  ``np.longdouble`` (64-bit significand on x86-64) with pairwise sums: about 2^-11 of a float64 ulp of
  error per element, so that each form's own float64 error model can be checked per element.

Notation: ``a`` is the correlated series of one column -- v (VACF), P = (m v) x (Helfand), x - x[0] (MSD),
q (x - x[0]) (conductivity self term), the moment M (Phi).  C(k) = sum_i a_i a_{i+k}, S(k) = sum_i (a_i - a_{i+k})^2 =
S1(k) - 2 C(k) with S1(k) = sum_{i < T-k} a_i^2 + sum_{i >= k} a_i^2.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53  # unit roundoff of float64
F64_EXACT = 2 ** 53
F32_EXACT = 2 ** 24

# ---------------------------------------------------------------------------------------------- the float32 budget
# What one float32 sum of the float32 paths takes before it is added into float64:
# * k_band32_tp (band32tp_kernels.hpp): kBand32tpFlush = 64 super-steps between flushes, 12 products per accumulator
#   element and super-step, on columns centred on a reference row (moved every 256 frames), so every operand is a
#   DIFFERENCE of two values of the series (|.| <= 2 max|a|) and every product <= 4 max|a|^2; the norm sums take as
#   many squares.  The flush (Band32Diag, band_common.hpp) then adds each diagonal of a 16 x 16 accumulator -- at
#   most 16 elements -- in float32 before the float64 add: 64 x 12 x 16 products in one float32 sum at most.
# * the float32 vector kernel (direct_kernels.hpp, chunk_accumulate on floats): 8 L-term float32 sums per lag (L <= 16:
#   128 squared differences or products, each <= 4 max|a|^2) before each float64 add -- below the matrix-core count.
BAND32TP_FLUSH, BAND32TP_PRODUCTS, BAND32TP_DIAGONAL = 64, 12, 16
F32_TERMS = BAND32TP_FLUSH * BAND32TP_PRODUCTS * BAND32TP_DIAGONAL


def budget(a, n_terms, f32=False):
    """Assert that the integer-valued series `a` keep every partial sum of the kernels exact, and return max|a|.

    Each term of a kernel's sum is a product or a squared difference of two values of a, or of two values centred on
    a third (the matrix-core forms), so |term| <= (2 max|a|)^2; no accumulator takes more than `n_terms` of them
    before it is rounded for good.  float64 paths: n_terms (2 max|a|)^2 < 2^53, with n_terms every term of a lag sum
    (n_cols x T) -- a bound for any order of summation.  float32 paths (f32=True): F32_TERMS (2 max|a|)^2 < 2^24, the
    count of one float32 sum between flushes (see F32_TERMS), and the float64 condition with n_terms as well."""
    a = np.asarray(a, dtype=np.float64)
    if not np.all(a == np.rint(a)):
        raise AssertionError("budget: the series is not integer-valued")
    amax = int(np.max(np.abs(a))) if a.size else 0
    checks = [(int(n_terms), F64_EXACT)] + ([(F32_TERMS, F32_EXACT)] if f32 else [])
    for n, limit in checks:
        bound = n * (2 * amax) ** 2
        if bound >= limit:
            raise AssertionError(f"budget: {n} terms of (2 x {amax})^2 = {bound} reach 2^{int(math.log2(limit))}")
    return amax


# ------------------------------------------------------------------------------------------------ integer inputs
def int_velocities(T, A, D, bound, seed):
    """Integer velocities uniform in [-bound, bound], float64 (T, A, D)."""
    rng = np.random.default_rng(seed)
    return rng.integers(-bound, bound + 1, size=(T, A, D)).astype(np.float64)


def int_walk(T, A, D, step, seed, drift=0, offset=0):
    """Integer random walks: steps uniform in [-step, step] plus `drift` per frame, from `offset` + a random integer in
    [0, 8 step]; float64 (T, A, D)."""
    rng = np.random.default_rng(seed)
    steps = rng.integers(-step, step + 1, size=(T, A, D)) + drift
    steps[0] = rng.integers(0, 8 * step + 1, size=(A, D))
    return np.cumsum(steps, axis=0).astype(np.float64) + offset


def int_masses(A, lo, hi, seed):
    """Integer masses uniform in [lo, hi]."""
    return np.random.default_rng(seed).integers(lo, hi + 1, size=A).astype(np.float64)


def int_charges(A, bound, seed):
    """Nonzero integer charges of magnitude 1 ... bound, half of each sign."""
    rng = np.random.default_rng(seed)
    q = rng.integers(1, bound + 1, size=A) * np.where(np.arange(A) % 2 == 0, 1, -1)
    return q[rng.permutation(A)].astype(np.float64)


# ------------------------------------------------------------------------------------------- exact numerators (int64)
def _as_int(a):
    a = np.asarray(a)
    ai = np.rint(a).astype(np.int64)
    if not np.array_equal(ai, a):
        raise ValueError("exact numerators need integer-valued series")
    return ai


def correlate_cols(a, fft_from=512, sample=4, seed=0):
    """C[k, c] = sum_{i < T-k} a[i, c] a[i+k, c] exactly (int64) for an integer-valued (T, n_cols) series.  Short series:
    int64 products lag by lag (up to 64 frames) or np.correlate per column.  From `fft_from` frames: rint of a float64
    FFT correlation, accepted only if every value lies within 1/8 of an integer and `sample` columns equal
    np.correlate."""
    ai = _as_int(a)
    T, n = ai.shape
    out = np.zeros((T, n), dtype=np.int64)
    if T <= 64:
        for k in range(T):
            out[k] = np.einsum("tc,tc->c", ai[:T - k], ai[k:])
        return out
    if T < fft_from:
        for c in range(n):
            out[:, c] = np.correlate(ai[:, c], ai[:, c], mode="full")[T - 1:]
        return out
    L = 1 << int(math.ceil(math.log2(2 * T)))
    f = np.fft.rfft(ai.astype(np.float64), n=L, axis=0)
    corr = np.fft.irfft(f.real ** 2 + f.imag ** 2, n=L, axis=0)[:T]
    r = np.rint(corr)
    dev = float(np.max(np.abs(corr - r))) if corr.size else 0.0
    if not dev < 0.125:
        raise AssertionError(f"FFT correlation lies {dev:g} from an integer: too far for an exact rint")
    out[:] = r.astype(np.int64)
    rng = np.random.default_rng(seed)
    for c in rng.choice(n, size=min(sample, n), replace=False):
        if not np.array_equal(out[:, c], np.correlate(ai[:, c], ai[:, c], mode="full")[T - 1:]):
            raise AssertionError(f"FFT correlation of column {c} differs from np.correlate")
    return out


def s1_cols(a):
    """S1[k, c] = sum_{i < T-k} a_i^2 + sum_{i >= k} a_i^2 (int64), from prefix sums."""
    ai = _as_int(a)
    T = ai.shape[0]
    p = np.zeros((T + 1,) + ai.shape[1:], dtype=np.int64)
    np.cumsum(ai * ai, axis=0, out=p[1:])
    k = np.arange(T)
    return p[T - k] + (p[T] - p[k])


def sqdiff_cols(a, **kw):
    """S[k, c] = sum_{i < T-k} (a_i - a_{i+k})^2 = S1 - 2 C (int64); S[0] = 0."""
    return s1_cols(a) - 2 * correlate_cols(a, **kw)


def per_particle(cols, A, D):
    """(T, A D) column numerators -> (T, A): each particle's D columns added."""
    return cols.reshape(cols.shape[0], A, D).sum(axis=2)


def vacf_num(v):
    """(T, A) numerators of the windowed VACF by particle: sum_d C_d(k)."""
    T, A, D = v.shape
    return per_particle(correlate_cols(v.reshape(T, A * D)), A, D)


def helfand_product(v, x, m):
    """P = (m v) x in the kernels' order; must be integer-valued."""
    P = (np.asarray(m, dtype=np.float64)[None, :, None] * v) * x
    _as_int(P)
    return P


def helfand_num(v, x, m):
    """(T, A) numerators of the Helfand by-particle array before scale / (D (T-k)): sum_d S_d(k) of P."""
    P = helfand_product(v, x, m)
    T, A, D = P.shape
    return per_particle(sqdiff_cols(P.reshape(T, A * D)), A, D)


def msd_num(x):
    """(T, A) numerators of the MSD by particle: sum_d S_d(k) of x - x[0]."""
    T, A, D = x.shape
    return per_particle(sqdiff_cols((x - x[0]).reshape(T, A * D)), A, D)


def moment_exact(x, q):
    """M[t, d] = sum_n q_n (x[t, n, d] - x[0, n, d]) (int64)."""
    return np.einsum("n,tnd->td", _as_int(q), _as_int(x - x[0]))


def phi_num(M):
    """(T,) numerators of Phi: sum_d S_d(k) of the moment."""
    return sqdiff_cols(M).sum(axis=1)


def species_moment_exact(y, q, labels, S, shift=True):
    """Q[s, t, d] = sum_{n: labels[n] = s} q_n (y[t, n, d] - y[0, n, d]) (int64, (S, T, D)): the species moments of
    positions; shift=False: the species currents sum q_n y[t, n, d] of velocities.  A label no atom carries: zeros."""
    y = np.asarray(y, dtype=np.float64)
    a = _as_int(y - y[0] if shift else y)
    qi, labels = _as_int(q), np.asarray(labels)
    Q = np.zeros((S,) + a.shape[:1] + a.shape[2:], dtype=np.int64)
    for s in range(S):
        sel = np.flatnonzero(labels == s)
        Q[s] = np.einsum("n,tnd->td", qi[sel], a[:, sel, :])
    return Q


def pseudo_particles(Q):
    """(T, S^2, D) int64: the series whose lag sums give the cross term by polarisation, pseudo-particle i S + j =
    Q_i (i == j), Q_i + Q_j (i < j), Q_i - Q_j (i > j), of integer-valued sums Q (S, T, D)."""
    Q = _as_int(Q)
    S, T, D = Q.shape
    P = np.empty((T, S * S, D), dtype=np.int64)
    for i in range(S):
        for j in range(S):
            P[:, i * S + j] = Q[i] if i == j else Q[i] + Q[j] if i < j else Q[i] - Q[j]
    return P


def pseudo_num(Q, acf=False, fft_from=1 << 30):
    """(T, S^2) numerators R[k, i S + j] of the pseudo-particles of Q (S, T, D): sum_d S_d(k) (the mean squared
    differences of moments), or with acf sum_d C_d(k) (the autocorrelations of currents).  Over T - k:
    C_ii = R[i S + i], C_ij = 1/4 (R[i S + j] - R[j S + i]) for i < j.  The sums of many atoms are large and their
    columns few, so the correlations are np.correlate's int64 sums at every length (`fft_from`: correlate_cols)."""
    P = pseudo_particles(Q)
    T, n, D = P.shape
    cols = P.reshape(T, n * D)
    return per_particle(correlate_cols(cols, fft_from=fft_from) if acf else sqdiff_cols(cols, fft_from=fft_from), n, D)


def self_num(x, q):
    """(T,) numerators of the Nernst-Einstein self term: sum_n q_n^2 sum_d S_nd(k)."""
    qi = _as_int(q)
    return msd_num(x) @ (qi * qi)


# ------------------------------------------------------------------------------------ correctly rounded expectations
def divide(num, den):
    """Correctly rounded float64 of num / den, elementwise (den: positive integers, broadcast against num): one IEEE
    division where both are exact in float64 (|.| < 2^53), else through Fraction."""
    num = np.asarray(num)
    den = np.broadcast_to(np.asarray(den, dtype=np.int64), num.shape)
    if num.dtype != object and np.all(np.abs(num) < F64_EXACT) and np.all(den < F64_EXACT):
        return num.astype(np.float64) / den.astype(np.float64)
    out = np.empty(num.shape)
    for idx in np.ndindex(num.shape):
        out[idx] = float(Fraction(int(num[idx]), int(den[idx])))
    return out


def lag_den(T):
    """(T,) T - k."""
    return T - np.arange(T, dtype=np.int64)


def ulps(got, want):
    """|got - want| in units of the last place of want; an exact match is 0, anything against an exact 0 is inf."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    diff = np.abs(got - want)
    zero = want == 0.0
    with np.errstate(invalid="ignore"):
        return np.where(zero, np.where(diff == 0.0, 0.0, np.inf), diff / np.where(zero, 1.0, np.spacing(np.abs(want))))


# ------------------------------------------------------------------------------ extended precision for float inputs
def longdouble_ok():
    """np.longdouble carries at least a 64-bit significand (x86-64 extended precision)."""
    return np.finfo(np.longdouble).nmant >= 63


def ld_corr(a, lags):
    """(len(lags), n_cols) sum_i a_i a_{i+k} per column of a (T, n_cols) series in np.longdouble (pairwise np.sum)."""
    a = np.asarray(a, dtype=np.float64).astype(np.longdouble)
    T = a.shape[0]
    out = np.zeros((len(lags),) + a.shape[1:], dtype=np.longdouble)
    for j, k in enumerate(lags):
        out[j] = np.sum(a[:T - k] * a[k:], axis=0)
    return out


def ld_sqdiff(a, lags):
    """(len(lags), n_cols) sum_i (a_i - a_{i+k})^2 per column in np.longdouble, difference first."""
    a = np.asarray(a, dtype=np.float64).astype(np.longdouble)
    T = a.shape[0]
    out = np.zeros((len(lags),) + a.shape[1:], dtype=np.longdouble)
    for j, k in enumerate(lags):
        if k:
            d = a[k:] - a[:T - k]
            out[j] = np.sum(d * d, axis=0)
    return out


def abs_corr(a, lags):
    """(len(lags), n_cols) sum_i |a_i a_{i+k}|: the condition scale of a correlation (float64)."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    T = a.shape[0]
    out = np.zeros((len(lags),) + a.shape[1:])
    for j, k in enumerate(lags):
        out[j] = np.sum(a[:T - k] * a[k:], axis=0)
    return out


def to_fraction(x):
    """An exact Fraction of a float64 or np.longdouble scalar."""
    return Fraction(*np.longdouble(x).as_integer_ratio())


def frac_corr(col, k):
    """sum_i a_i a_{i+k} of one float64 column in exact rational arithmetic."""
    f = [Fraction(float(t)) for t in col]
    return sum((f[i] * f[i + k] for i in range(len(f) - k)), Fraction(0))


def frac_sqdiff(col, k):
    """sum_i (a_i - a_{i+k})^2 of one float64 column in exact rational arithmetic."""
    f = [Fraction(float(t)) for t in col]
    return sum(((f[i] - f[i + k]) ** 2 for i in range(len(f) - k)), Fraction(0))


# ------------------------------------------------------------------------------------------------ FFT error model
FFT_C = 16


def column_energy(a):
    """sum_t a_t^2 of a (T, ...) series: one energy per column."""
    a = np.asarray(a, dtype=np.float64)
    return np.einsum("t...,t...->...", a, a)


def fft_energy_bp(e_particle):
    """E of each by-particle element of the FFT forms: the energy of every column whose data passes through a transform
    that the particle's data passes through.  In wfft.hpp two particles 2m and 2m + 1 meet in two places: the one-pass
    by-particle kernel (k_w1_bp, up to 256 frames) inverts the power spectra of 2m and 2m + 1 as ONE complex transform
    (of P_a + i P_b), and the multi-pass forward kernel (k_wbp) with an odd number of columns per particle transforms
    the column pair that 2m and 2m + 1 share as one complex series.  Nowhere else: a particle's units are its own
    columns (the two units of a D = 3 particle, one transform up to 128 frames, are both its own), the packed short
    plans (2 / 4 / 8 column pairs in one transform) serve the lag sums alone, and the CPU backend pairs atoms 2m and
    2m + 1 the same way.  So E_n = e_2m + e_2m+1 with m = n // 2 (e_n alone for an unpaired last particle).
    e_particle: (A,) energies sum_d sum_t a^2 per particle."""
    e = np.asarray(e_particle, dtype=np.float64)
    n_even = e.shape[0] - (e.shape[0] & 1)
    out = e.copy()
    out[:n_even] = e[:n_even].reshape(-1, 2).sum(axis=1).repeat(2)
    return out


def fft_bound(T, L, E, S1=None, C=FFT_C):
    """Per-lag bound of FFT-form elements: [C u log2(L) E + 4 u S1(k)] / (T - k), shape (T,) + E.shape.  E: the energy
    through the element's transforms (a scalar, or (A,) by particle); S1: (T,) + E.shape, the window's sum |a|^2 over
    the element's own columns for the S1 - 2 S2 forms, else None."""
    E = np.asarray(E, dtype=np.float64)
    S1 = np.zeros((T,) + E.shape) if S1 is None else np.asarray(S1, dtype=np.float64)
    den = lag_den(T).astype(np.float64).reshape((T,) + (1,) * E.ndim)
    return (C * U * math.log2(L) * E + 4 * U * S1) / den


def s1_float(a):
    """S1(k) per column of a float (T, ...) series, float64 (for the FFT bound only)."""
    a2 = np.asarray(a, dtype=np.float64) ** 2
    T = a2.shape[0]
    p = np.concatenate([np.zeros((1,) + a2.shape[1:]), np.cumsum(a2, axis=0)])
    k = np.arange(T)
    return p[T - k] + (p[T] - p[k])


# ----------------------------------------------------------------------- k-space: quarter-turn phases (scattering, currents)
# Integer positions and wavevectors k = 2 pi q with every component of q a multiple of 1/4: u = q . x is an exact multiple
# of 1/4 in float64, r = u - rint(u) one of 0, +-1/4, +-1/2, and exp(2 pi i r) one of 1, i, -1, -i.  Every density,
# current and lag-sum numerator behind such phases is an integer.
TWO_PI = 6.283185307179586476925  # the literal of phase_math.hpp (it rounds to float64's 2 pi)
QUARTER_COS = np.array([1, 0, -1, 0], dtype=np.int64)
QUARTER_SIN = np.array([0, 1, 0, -1], dtype=np.int64)


def quarter_wavevectors(q):
    """k = q 2 pi (rad per length unit) of turns q whose components are multiples of 1/4; asserts that the library's
    k / 2 pi gives q back in float64 (it does for the multiples of 1/4 in [-2.5, 2.5] and +-3, +-3.5, +-4; not for
    +-2.75, +-3.25, +-3.75)."""
    q = np.asarray(q, dtype=np.float64)
    _as_int(4 * q)
    k = q * TWO_PI
    back = k / TWO_PI
    if not np.array_equal(back, q):
        bad = q[back != q]
        raise AssertionError(f"k / 2 pi does not give q back for q = {sorted(set(bad.ravel().tolist()))}")
    return k


def quarter_phases(x, q):
    """(K, T, A) int64 in 0 ... 3: the phase of exp(i k_j . x[t, n]) in quarter turns, for integer positions x (T, A, D)
    and turns q (K, D) that are multiples of 1/4."""
    return np.einsum("kd,tnd->ktn", _as_int(4 * np.asarray(q, dtype=np.float64)), _as_int(x)) % 4


def quarter_cs(x, q):
    """((K, T, A), (K, T, A)) int64: cos and sin of the quarter-turn phases, each one of 1, 0, -1."""
    p = quarter_phases(x, q)
    return QUARTER_COS[p], QUARTER_SIN[p]


def pair_acf_num(a):
    """(T, P) numerators sum_i a[i, p] . a[i + k, p] of an integer-valued (T, P, C) series: the autocorrelation of every
    pseudo-atom p over its C columns (vacf_num under another name, for series that are no velocities)."""
    return vacf_num(np.asarray(a, dtype=np.float64))


def scatter_exact(x, q):
    """The exact integers behind ta_scatter at quarter-turn phases: (density (K, T, 2) int64 = sum_n (cos, sin),
    self numerators by atom (K, T, A) = sum_t cos(phi[t + k, n] - phi[t, n]), coll numerators (K, T) = the autocorrelation
    of the density)."""
    c, s = quarter_cs(x, q)
    rho = np.stack([c.sum(axis=2), s.sum(axis=2)], axis=2)
    self_num = np.stack([pair_acf_num(np.stack([cj, sj], axis=2)) for cj, sj in zip(c, s)])
    return rho, self_num, pair_acf_num(rho.transpose(1, 0, 2)).T


def current_exact(x, v, w, q):
    """(K, T, D, 2) int64: current[j, t, d] = sum_n w_n v[t, n, d] (cos, sin)(k_j . x[t, n]) at quarter-turn phases, for
    integer velocities and integer weights (None: ones)."""
    c, s = quarter_cs(x, q)
    wv = _as_int(v) * (1 if w is None else _as_int(w)[None, :, None])
    return np.stack([np.einsum("ktn,tnd->ktd", c, wv), np.einsum("ktn,tnd->ktd", s, wv)], axis=3)


def partial_exact(x, w, labels, S, q):
    """The exact integers behind ta_partial_density at quarter-turn phases, for integer positions x (T, A, D), integer
    weights w (None: ones), labels in 0 ... S - 1 and turns q (K, D): (density (K, S, T, 2) int64 = sum_{n in a} w_n (cos,
    sin) -- a label nobody carries: zeros --, numerators (K, T, S^2) int64 of the autocorrelations of each wavevector's S^2
    pseudo-particles in slab order: pseudo-particle i S + j is rho_i (i == j), rho_i + rho_j (i < j), rho_i - rho_j (i > j),
    as k_onsager_combos lays them out).  Over T - k: cross_aa = num[a S + a], cross_ab = 1/4 (num[a S + b] - num[b S + a])
    for a < b."""
    c, s = quarter_cs(x, q)
    wi = np.ones(c.shape[2], dtype=np.int64) if w is None else _as_int(w)
    labels = np.asarray(labels)
    K, T, _ = c.shape
    rho = np.zeros((K, S, T, 2), dtype=np.int64)
    for a in range(S):
        sel = np.flatnonzero(labels == a)
        rho[:, a, :, 0] = c[:, :, sel] @ wi[sel]
        rho[:, a, :, 1] = s[:, :, sel] @ wi[sel]
    num = np.stack([pair_acf_num(pseudo_particles(rho[j])) for j in range(K)]) if K else np.zeros((0, T, S * S), dtype=np.int64)
    return rho, num


def axis_current_num(cur, axis):
    """(long numerators (T,), transverse numerators by component (T, D)) of one wavevector's integer current (T, D, 2) when
    the wavevector has ONE non-zero component `axis`: k^ = +-e_axis exactly, jL = +-current[axis], jT[d] = current[d] for
    d != axis and exactly 0 for d = axis.  trans = sum_d of the second / ((D - 1) (T - k))."""
    num = pair_acf_num(cur)  # (T, D)
    tr = num.copy()
    tr[:, axis] = 0
    return num[:, axis], tr


# ------------------------------------------------------------------------------- axis-aligned molecules (orientation)
def axis_molecules(T, N, mode, seed, hop=0.15, degenerate=0.04, box=None):
    """Molecules (a, b, c) of integer positions whose orientation vector is exactly +-e_x, +-e_y or +-e_z times an integer
    length, hopping between the six directions with probability `hop` per frame, and degenerate (no direction) in a
    fraction `degenerate` of the (frame, molecule) pairs.  mode "bond": b - a = L e; "normal": b - a = L1 e_i, c - a =
    L2 e_j, v = L1 L2 e_i x e_j; "bisector": b - a = p e + q e', c - a = p e - q e' (e' another axis), v = 2 p e.
    box: None, or (T,) integer box lengths (cubic; every arm is shorter than a quarter of the smallest): the atoms are
    wrapped into [0, box) one by one, so that the image step has work to do.
    -> (x (T, 3 N, 3) float64 integers, index (N, 2 or 3) int32 in a permuted order, u (T, N, 3) int64 in {-1, 0, 1})."""
    rng = np.random.default_rng(seed)
    direction = np.empty((T, N), dtype=np.int64)  # 0 ... 5: +x, -x, +y, -y, +z, -z
    direction[0] = rng.integers(0, 6, size=N)
    hops = rng.random((T, N)) < hop
    fresh = rng.integers(0, 6, size=(T, N))
    for t in range(1, T):
        direction[t] = np.where(hops[t], fresh[t], direction[t - 1])
    axis, sign = direction // 2, 1 - 2 * (direction % 2)
    live = rng.random((T, N)) >= degenerate
    e = np.zeros((T, N, 3), dtype=np.int64)
    np.put_along_axis(e, axis[:, :, None], sign[:, :, None], axis=2)
    a = np.rint(np.cumsum(rng.integers(-1, 2, size=(T, N, 3)), axis=0) + rng.integers(0, 9, size=(1, N, 3))).astype(np.int64)
    L1 = rng.integers(1, 4, size=(T, N, 1))
    L2 = rng.integers(1, 4, size=(T, N, 1))
    if mode == "bond":
        db, dc = L1 * e * live[:, :, None], np.zeros_like(e)
    elif mode == "bisector":
        other = np.zeros_like(e)  # a unit vector along the next axis
        np.put_along_axis(other, ((axis + 1) % 3)[:, :, None], 1, axis=2)
        p = L1 * live[:, :, None]  # degenerate: p = 0, the arms opposite
        db, dc = p * e + L2 * other, p * e - L2 * other
    else:
        assert mode == "normal"
        e_i = np.zeros_like(e)
        e_j = np.zeros_like(e)
        np.put_along_axis(e_i, ((axis + 1) % 3)[:, :, None], 1, axis=2)
        np.put_along_axis(e_j, ((axis + 2) % 3)[:, :, None], 1, axis=2)
        db = L1 * e_i
        dc = np.where(live[:, :, None], L2 * sign[:, :, None] * e_j, 2 * db)  # degenerate: parallel arms
    x = np.stack([a, a + db, a + dc], axis=2).reshape(T, 3 * N, 3)
    if box is not None:
        x = x % np.asarray(box, dtype=np.int64).reshape(T, 1, 1)
    order = rng.permutation(N)
    rows = np.stack([3 * order, 3 * order + 1] + ([] if mode == "bond" else [3 * order + 2]), axis=1)
    u = (e * live[:, :, None])[:, order]
    return x.astype(np.float64), np.ascontiguousarray(rows, dtype=np.int32), u


def orient_exact(u, w=None):
    """The exact integers behind ta_orient for unit vectors u (T, N, 3) in {-1, 0, 1} (one non-zero component, or none):
    (c1 numerators by vector (T, N) = sum_t u . u', n_same (T,), n_diff (T,): the pairs (t, t + k) of one vector, both
    with a direction, along the same axis / along different axes -- c2[k] = (2/3 n_same - 1/3 n_diff) / (T - k) --,
    total (T, 3) int64 = sum_n w_n u_n with integer weights, coll numerators (T,))."""
    u = _as_int(u)
    same = pair_acf_num(np.abs(u)).sum(axis=1)
    live = np.abs(u).sum(axis=2, keepdims=True)
    both = pair_acf_num(live).sum(axis=1)
    total = np.einsum("n,tnd->td", np.ones(u.shape[1], dtype=np.int64) if w is None else _as_int(w), u)
    return pair_acf_num(u), same, both - same, total, pair_acf_num(total[:, None, :])[:, 0]
