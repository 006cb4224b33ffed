"""Long-double reference of the current correlation functions, written from the definitions of include/ta_hip.h
(ta_kcurrent) and independent of the library:

    phi_j[t, n]        = sum_d k_j[d] x[t, n, d]
    current[j, t, d]   = ( sum_n w_n v[t, n, d] cos phi_j[t, n],  sum_n w_n v[t, n, d] sin phi_j[t, n] )
    k^_j = k_j / |k_j|;  jL[j, t] = sum_d k^_j[d] current[j, t, d];  jT[j, t, d] = current[j, t, d] - k^_j[d] jL[j, t]
    long[j, tau]       = 1/(T - tau) sum_{t < T - tau} Re(conj(jL[j, t]) jL[j, t + tau])
    trans[j, tau]      = 1/(D - 1) 1/(T - tau) sum_{t < T - tau} sum_d Re(conj(jT[j, t, d]) jT[j, t + tau, d])   (D = 1: zeros)

x, v: the float64 values actually staged (both exact in float32: scatter_ref's walk on the 1/1024 grid, and an independent
draw of velocities on the same grid); w: dyadic weights.  The lag sums are direct sums at scatter_ref's lag_sample.

The bars.  current, first order in u_r = 2^-53: each component d lies within S_d (2 pi (D + 2) u_r U + (10 + A) u_r) of
the exact sum, S_d = max_t sum_n |w_n v[t, n, d]|, U = max |k . x| / (2 pi) -- the phase rounding (D products and sums and
the reduction, times 2 pi), 8 u_r for the math functions, 2 for the two products, A u_r for a sum of A terms in any order.
long and trans: each within 1e-10 (the project's standing bar of a correlation stage) of max |long + (D - 1) trans| over
the lags and wavevectors -- the trace, so that a series that is zero by symmetry has a scale -- against the long-double
projection and autocorrelation of the RETURNED current."""
import functools

import numpy as np

from scatter_ref import LD, U_R, lag_sample, phases, unit_scale, walk, wavevectors

WEIGHTS = np.array([0.5, 1.0, 2.0, -1.0, 0.25, 4.0])


def velocities(T, A, D, seed, scale=0.5):
    """an independent normal draw on the 1/1024 grid: exact in float32"""
    rng = np.random.default_rng(seed + 2000)
    return np.rint(rng.normal(scale=scale * 1024, size=(T, A, D))) / 1024.0


def weights(A, seed):
    return WEIGHTS[np.random.default_rng(seed + 3000).integers(0, WEIGHTS.size, size=A)]


def current_of(x, v, w, k):
    """(K, T, D, 2) long double"""
    ph = phases(x, k)
    wv = np.asarray(v, dtype=LD) * (np.ones(np.shape(v)[1], dtype=LD) if w is None else np.asarray(w, dtype=LD))[None, :, None]
    re = np.einsum("ktn,tnd->ktd", np.cos(ph), wv)
    im = np.einsum("ktn,tnd->ktd", np.sin(ph), wv)
    return np.stack([re, im], axis=3)


def current_bar(x, v, w, k):
    """(D,) the bound on either part of component d of the current"""
    T, A, D = np.shape(x)
    ww = np.ones(A) if w is None else np.asarray(w, dtype=np.float64)
    S = np.max(np.sum(np.abs(np.asarray(v) * ww[None, :, None]), axis=1), axis=0)
    return S * (2 * np.pi * (D + 2) * U_R * unit_scale(x, k) + (10 + A) * U_R)


def project(current, k):
    """jL (K, T, 2), jT (K, T, D, 2) of a (K, T, D, 2) current, in long double"""
    cur = np.asarray(current, dtype=LD)
    kk = np.asarray(k, dtype=LD)
    kh = kk / np.sqrt((kk * kk).sum(axis=1))[:, None]
    jl = np.einsum("kd,ktdh->kth", kh, cur)
    return jl, cur - kh[:, None, :, None] * jl[:, :, None, :]


def acf_at(a, lags):
    """(K, len(lags)): 1/(T - tau) sum_t of the products a[:, t] a[:, t + tau] summed over every axis behind the time axis"""
    K, T = a.shape[:2]
    out = np.zeros((K, len(lags)), dtype=LD)
    for i, tau in enumerate(lags):
        n = T - int(tau)
        out[:, i] = (a[:, :n] * a[:, int(tau):]).reshape(K, -1).sum(axis=1) / n
    return out


def correlations_at(current, k, lags):
    """(long, trans) (K, len(lags)) of a (K, T, D, 2) current (e.g. the one a call returned), in long double"""
    D = np.shape(current)[2]
    jl, jt = project(current, k)
    lon = acf_at(jl, lags)
    return lon, (acf_at(jt, lags) / (D - 1) if D > 1 else np.zeros_like(lon))


@functools.lru_cache(maxsize=48)
def case(T, A, D, K, seed=1, weighted=True):
    """(x, v, w or None, k, lags, current, bar): computed once and shared; not to be modified"""
    x, v, k = walk(T, A, D, seed), velocities(T, A, D, seed), wavevectors(K, D, seed)
    w = weights(A, seed) if weighted else None
    for a in (x, v):
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
    out = (x, v, w, k, lag_sample(T), current_of(x, v, w, k), current_bar(x, v, w, k))
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def assert_current(got, ref, what="", slack=1.0):
    """a returned current against case(...)'s: every component within its bar (slack: 2 for the sum of two bars)"""
    cur, bar = ref[5], ref[6]
    err = np.max(np.abs(np.asarray(got, dtype=LD) - cur), axis=(0, 1, 3)).astype(np.float64)
    print(f"    {what} current: {err} (bar {slack * bar})")
    assert np.all(err <= slack * bar), (what, err, slack * bar)


def assert_correlations(got_current, got_long, got_trans, ref, what=""):
    """long / trans of a call against the long-double correlations of the current it RETURNED, at case(...)'s lags; every
    figure printed before it is asserted"""
    k, lags = ref[3], ref[4]
    D = np.shape(got_current)[2]
    lon, tr = correlations_at(got_current, k, lags)
    scale = float(np.max(np.abs(lon + (D - 1) * tr)))
    for name, got, want in (("long", got_long, lon), ("trans", got_trans, tr)):
        if got is None:
            continue
        err = float(np.max(np.abs(np.asarray(got, dtype=LD)[:, lags] - want)))
        print(f"    {what} {name}: {err:.3e} ({err / scale if scale else 0.0:.3e} of {scale:.3e})")
        assert err <= 1e-10 * scale, (what, name, err, scale)
    if D == 1 and got_trans is not None:
        assert not np.any(got_trans), "D = 1: trans is zeros"


def assert_kcurrent(got_current, got_long, got_trans, ref, what=""):
    assert_current(got_current, ref, what)
    assert_correlations(got_current, got_long, got_trans, ref, what)
