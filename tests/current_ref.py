"""References for the Green-Kubo tests, in NumPy long double: the species currents as plain sums, and their symmetrised
cross-correlation as direct sums, lag by lag.  Nothing here knows about polarisation or transforms."""
import functools

import numpy as np

LD = np.longdouble


def species_velocities(T, A, S, seed, D=3):
    """(v, labels, weights): normal velocities with a slowly varying part shared by an atom's frames (so that the
    correlations do not vanish at once); labels 0 ... S - 1 in random order with UNEQUAL species sizes -- species 0 holds
    about 70 % of the atoms, every species at least one when A >= S -- and weights from {-1, 0.5, 1, 2}."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((T, A, D)) + 0.5 * np.cos(0.01 * np.arange(T))[:, None, None] * rng.standard_normal((1, A, D))
    lab = np.where(rng.random(A) < 0.7, 0, rng.integers(1, max(S, 2), size=A)) if S > 1 else np.zeros(A, dtype=np.int64)
    lab[:min(S, A)] = np.arange(min(S, A))  # nobody is missing
    lab = rng.permutation(lab).astype(np.int32)
    w = rng.choice([-1.0, 0.5, 1.0, 2.0], size=A)
    return v, lab, w


def currents_ref(v, lab, w, S):
    """(J (S, T, D) long double, scale (S, T)): J_s = sum_{n in s} w_n v, scale[s, t] = sum_{n in s} |w_n| sum_d |v|: what
    the error of J_s[t] is relative to, per species and frame."""
    v = np.asarray(v, dtype=np.float64)
    T, A, D = v.shape
    w = np.ones(A) if w is None else np.asarray(w, dtype=np.float64)
    J = np.zeros((S, T, D), dtype=LD)
    scale = np.zeros((S, T))
    for s in range(S):
        sel = np.flatnonzero(np.asarray(lab) == s)
        if sel.size:
            term = v[:, sel, :].astype(LD) * w[sel].astype(LD)[None, :, None]
            J[s] = term.sum(axis=1)
            scale[s] = np.abs(term).sum(axis=(1, 2)).astype(np.float64)
    return J, scale


def cross_ref(J):
    """C (T, S, S) long double of currents J (S, T, D): C[k, i, j] = 1/2 mean_t sum_d (J_i[t] J_j[t+k] + J_j[t] J_i[t+k]),
    lag 0 included."""
    J = np.asarray(J, dtype=LD)
    S, T, D = J.shape
    C = np.zeros((T, S, S), dtype=LD)
    for k in range(T):
        a = np.einsum("itd,jtd->ij", J[:, :T - k, :], J[:, k:, :]) / LD(T - k)
        C[k] = LD(0.5) * (a + a.T)
    return C


def cross_at_lags(J, lags):
    """cross_ref(J)[lags], (len(lags), S, S) long double, without the other lags' work."""
    J = np.asarray(J, dtype=LD)
    S, T, D = J.shape
    C = np.zeros((len(lags), S, S), dtype=LD)
    for n, k in enumerate(lags):
        a = np.einsum("itd,jtd->ij", J[:, :T - k, :], J[:, k:, :]) / LD(T - k)
        C[n] = LD(0.5) * (a + a.T)
    return C


def pair_scale(C):
    """(S, S): max(C_ii(0), C_jj(0)), what the error of C_ij is relative to."""
    diag = np.abs(np.einsum("ii->i", np.asarray(C[0], dtype=np.float64)))
    return np.maximum(diag[:, None], diag[None, :])


def assert_currents(got, want, scale, tol=1e-12):
    got = np.asarray(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got.astype(LD) - want).max(axis=2).astype(np.float64)  # (S, T)
    empty = scale == 0.0
    assert not err[empty].any(), "no atoms, or all velocities zero: the current must be exactly zero"
    worst = float((err[~empty] / scale[~empty]).max()) if (~empty).any() else 0.0
    print(f"    J: worst error {worst:.3e} of sum |w| |v|")
    assert worst <= tol, f"currents: {worst:.3e} of sum |w| |v|"


def assert_cross(got, want, tol=1e-10):
    got = np.asarray(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, got.transpose(0, 2, 1)), "C must be symmetric bit for bit"
    scale = pair_scale(want)
    err = np.abs(got.astype(LD) - want).max(axis=0).astype(np.float64)
    worst = np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), err)
    print(f"    C: worst pair error {worst.max():.3e} of max(C_ii(0), C_jj(0))")
    assert (worst <= tol).all(), f"C: {worst.max():.3e} of max(C_ii(0), C_jj(0)) at pair {np.unravel_index(worst.argmax(), worst.shape)}"


@functools.lru_cache(maxsize=8)
def velocity_case(T, A, S, D=3, f32=False):
    """species_velocities(T, A, S, seed = T + A + S) with its references: (v, lab, w, J, scale, C); f32: of the velocities
    rounded to float32 first."""
    v, lab, w = species_velocities(T, A, S, seed=T + A + S, D=D)
    if f32:
        v = v.astype(np.float32).astype(np.float64)
    J, scale = currents_ref(v, lab, w, S)
    for a in (v, lab, w):
        a.setflags(write=False)
    return v, lab, w, J, scale, cross_ref(J)
