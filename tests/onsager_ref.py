"""References for the Onsager tests, in NumPy long double: the species moments as plain sums, and the cross mean squared
displacement difference first, lag by lag.  Nothing here knows about polarisation or transforms."""
import functools

import numpy as np

LD = np.longdouble


def species_walk(T, A, S, seed, D=3, drift=0.0):
    """(x, labels, weights): random walks 1000 away from the origin, like unwrapped positions (`drift`: one more walk
    shared by every atom, that many times an atom's own step); labels 0 ... S - 1 in random order with UNEQUAL species
    sizes -- species 0 holds about 70 % of the atoms, every species at least one when A >= S -- and weights from
    {0.5, 1, 2}."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.standard_normal((T, A, D)), axis=0) + 1000.0
    if drift:
        x += drift * np.cumsum(rng.standard_normal((T, 1, D)), axis=0)
    lab = np.where(rng.random(A) < 0.7, 0, rng.integers(1, max(S, 2), size=A)) if S > 1 else np.zeros(A, dtype=np.int64)
    lab[:min(S, A)] = np.arange(min(S, A))  # nobody is missing
    lab = rng.permutation(lab).astype(np.int32)
    w = rng.choice([0.5, 1.0, 2.0], size=A)
    return x, lab, w


def moments_ref(x, lab, w, S):
    """(M (S, T, D) long double, scale (S,)): M_s = sum_{n in s} w_n (x - x[0]), scale_s = max_{t, d} sum_{n in s} |w_n| |x - x[0]|."""
    x = np.asarray(x, dtype=np.float64)
    T, A, D = x.shape
    w = np.ones(A) if w is None else np.asarray(w, dtype=np.float64)
    dx = x.astype(LD) - x[0].astype(LD)
    M = np.zeros((S, T, D), dtype=LD)
    scale = np.zeros(S)
    for s in range(S):
        sel = np.flatnonzero(np.asarray(lab) == s)
        if sel.size:
            term = dx[:, sel, :] * w[sel].astype(LD)[None, :, None]
            M[s] = term.sum(axis=1)
            scale[s] = float(np.abs(term).sum(axis=1).max())
    return M, scale


def cross_ref(M):
    """C (T, S, S) long double of moments M (S, T, D): C[k, i, j] = mean_t sum_d (M_i[t+k] - M_i[t]) (M_j[t+k] - M_j[t])."""
    M = np.asarray(M, dtype=LD)
    S, T, D = M.shape
    C = np.zeros((T, S, S), dtype=LD)
    for k in range(1, T):
        d = M[:, k:, :] - M[:, :-k, :]
        C[k] = np.einsum("itd,jtd->ij", d, d) / LD(T - k)
    return C


def cross_at_lags(M, lags):
    """cross_ref(M)[lags], (len(lags), S, S) long double, without the other lags' work."""
    M = np.asarray(M, dtype=LD)
    S, T, D = M.shape
    C = np.zeros((len(lags), S, S), dtype=LD)
    for n, k in enumerate(lags):
        if k:
            d = M[:, k:, :] - M[:, :T - k, :]
            C[n] = np.einsum("itd,jtd->ij", d, d) / LD(T - k)
    return C


def pair_scale(C):
    """(S, S): max_k max(C_ii, C_jj), what the error of C_ij is relative to."""
    C = np.asarray(C, dtype=np.float64)
    diag = np.abs(np.einsum("kii->ki", C)).max(axis=0)
    return np.maximum(diag[:, None], diag[None, :])


def assert_moments(got, want, scale, tol=1e-12):
    got = np.asarray(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    for s in range(want.shape[0]):
        err = float(np.abs(got[s].astype(LD) - want[s]).max())
        if scale[s] == 0.0:
            assert err == 0.0, f"species {s} has no atoms: its moment must be exactly zero"
        else:
            assert err <= tol * scale[s], f"moment of species {s}: {err / scale[s]:.3e} of scale"


def assert_cross(got, want, tol=1e-10):
    got = np.asarray(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert not got[0].any(), "lag 0 must be exactly 0"
    assert np.array_equal(got, got.transpose(0, 2, 1)), "C must be symmetric bit for bit"
    scale = pair_scale(want)
    err = np.abs(got.astype(LD) - want).max(axis=0).astype(np.float64)
    worst = np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), err)
    print(f"    C: worst pair error {worst.max():.3e} of max(C_ii, C_jj)")
    assert (worst <= tol).all(), f"C: {worst.max():.3e} of max(C_ii, C_jj) at pair {np.unravel_index(worst.argmax(), worst.shape)}"


@functools.lru_cache(maxsize=8)
def walk_case(T, A, S, D=3, drift=0.0, f32=False):
    """species_walk(T, A, S, seed = T + A + S) with its references: (x, lab, w, M, scale, C); f32: of the positions
    rounded to float32 first."""
    x, lab, w = species_walk(T, A, S, seed=T + A + S, D=D, drift=drift)
    if f32:
        x = x.astype(np.float32).astype(np.float64)
    M, scale = moments_ref(x, lab, w, S)
    for a in (x, lab, w):
        a.setflags(write=False)
    return x, lab, w, M, scale, cross_ref(M)
