"""Long-double reference of the partial scattering functions, written from the definitions of include/ta_hip.h
(ta_partial_density) and independent of the library:

    phi_j[t, n]         = sum_d k_j[d] x[t, n, d]
    rho[j, a, t]        = sum_{n: species[n] = a} w_n (cos phi_j[t, n], sin phi_j[t, n])
    cross[j, tau, a, b] = 1/2 1/(T - tau) sum_{t < T - tau} Re(conj(rho[j, a, t]) rho[j, b, t + tau] + conj(rho[j, b, t]) rho[j, a, t + tau])

x: the float64 values actually staged (exact in float32: scatter_ref's walk on the 1/1024 grid); w: kcurrent_ref's dyadic
weights, so every weighted term is exact; labels: interleaved (n mod S), with `empty` a species that gets no atom.  The lag
sums are direct sums at scatter_ref's lag_sample.

The bars.  density, first order in u_r = 2^-53: each component of species a lies within W_a (2 pi (D + 2) u_r U + (10 + n_a)
u_r) of the exact sum, W_a = sum_{n in a} |w_n|, n_a its atoms, U = max |k . x| / (2 pi) -- the phase rounding (D products
and sums and the reduction, times 2 pi), 8 u_r for the math functions, 2 for the fma's product, n_a u_r for a sum of n_a
terms in any order.  cross: each element (a, b) of wavevector j within 1e-10 (the project's standing bar of a correlation
stage) of max(cross[j, 0, a, a], cross[j, 0, b, b]) -- NOT of |cross[j, tau, a, b]|: an off-diagonal element is a difference
of two autocorrelations of that size -- against the defining sum, in long double, of the RETURNED density."""
import functools

import numpy as np

from kcurrent_ref import weights
from scatter_ref import LD, U_R, lag_sample, phases, unit_scale, walk, wavevectors


def labels(A, S, empty=None):
    """interleaved labels n mod S; `empty`: that species' atoms go to the next one (S >= 2), so it stays without atoms"""
    lab = (np.arange(A) % S).astype(np.int32)
    if empty is not None:
        lab[lab == empty] = (empty + 1) % S
    return lab


def density_of(x, w, lab, S, k):
    """(K, S, T, 2) long double"""
    ph = phases(x, k)
    ww = np.ones(np.shape(x)[1], dtype=LD) if w is None else np.asarray(w, dtype=LD)
    c, s = np.cos(ph) * ww, np.sin(ph) * ww
    out = np.zeros((ph.shape[0], S, ph.shape[1], 2), dtype=LD)
    for a in range(S):
        sel = lab == a
        out[:, a, :, 0], out[:, a, :, 1] = c[:, :, sel].sum(axis=2), s[:, :, sel].sum(axis=2)
    return out


def density_bar(x, w, lab, S, k):
    """(S,) the bound on either part of species a's density"""
    T, A, D = np.shape(x)
    ww = np.ones(A) if w is None else np.abs(np.asarray(w, dtype=np.float64))
    W = np.bincount(lab, weights=ww, minlength=S)
    n = np.bincount(lab, minlength=S)
    return W * (2 * np.pi * (D + 2) * U_R * unit_scale(x, k) + (10 + n) * U_R)


def cross_at(density, lags):
    """(K, len(lags), S, S) of a (K, S, T, 2) density (e.g. the one a call returned): the defining sum in long double"""
    rho = np.asarray(density, dtype=LD)
    K, S, T, _ = rho.shape
    out = np.zeros((K, len(lags), S, S), dtype=LD)
    for i, tau in enumerate(lags):
        n = T - int(tau)
        p = np.einsum("kath,kbth->kab", rho[:, :, :n], rho[:, :, int(tau):]) / n  # Re(conj(rho_a[t]) rho_b[t + tau])
        out[:, i] = (p + p.transpose(0, 2, 1)) / 2
    return out


@functools.lru_cache(maxsize=64)
def case(T, A, D, K, S, seed=1, weighted=True, empty=None):
    """(x, w or None, labels, k, lags, density, bar, S): computed once and shared; not to be modified"""
    x, k, lab = walk(T, A, D, seed), wavevectors(K, D, seed), labels(A, S, empty)
    w = weights(A, seed) if weighted else None
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    out = (x, w, lab, k, lag_sample(T), density_of(x, w, lab, S, k), density_bar(x, w, lab, S, k), S)
    for a in out[:7]:
        if a is not None:
            a.setflags(write=False)
    return out


def assert_density(got, ref, what="", slack=1.0):
    """a returned density against case(...)'s: every species within its bar (slack: 2 for the sum of two bars); a species
    without atoms: exact zeros"""
    lab, rho, bar, S = ref[2], ref[5], ref[6], ref[7]
    assert np.shape(got) == rho.shape, (np.shape(got), rho.shape)
    err = np.max(np.abs(np.asarray(got, dtype=LD) - rho), axis=(0, 2, 3)).astype(np.float64)
    print(f"    {what} density: {err} (bar {slack * bar})")
    assert np.all(err <= slack * bar), (what, err, slack * bar)
    for a in range(S):
        if not np.any(lab == a):
            assert not np.any(np.asarray(got)[:, a]), (what, "an empty species' density is not exactly zero", a)


def assert_cross(got_density, got_cross, ref, what=""):
    """cross of a call against the defining sum of the density it RETURNED, at case(...)'s lags; symmetric bit for bit;
    exact zeros in the row and column of a species whose density is all zero; every figure printed before it is asserted"""
    lags, S = ref[4], ref[7]
    got = np.asarray(got_cross)
    assert got.shape == (np.shape(got_density)[0], np.shape(got_density)[2], S, S), got.shape
    assert np.array_equal(got, got.transpose(0, 1, 3, 2)), (what, "cross is not symmetric bit for bit")
    want = cross_at(got_density, lags)
    diag0 = np.einsum("kaa->ka", want[:, 0]) if lags[0] == 0 else None
    assert diag0 is not None
    scale = np.maximum(diag0[:, :, None], diag0[:, None, :]).astype(np.float64)  # (K, S, S)
    err = np.max(np.abs(got[:, lags].astype(LD) - want), axis=1).astype(np.float64)  # (K, S, S)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(scale > 0, err / scale, 0.0)
    print(f"    {what} cross: {float(np.max(err)):.3e} ({float(np.max(rel)):.3e} of max(cross_aa(0), cross_bb(0)))")
    assert np.all(err <= 1e-10 * scale), (what, float(np.max(rel)))
    for a in range(S):
        if not np.any(np.asarray(got_density)[:, a]):
            assert not np.any(got[:, :, a, :]) and not np.any(got[:, :, :, a]), (what, "an empty species' cross terms are not zero", a)


def assert_partial(got_density, got_cross, ref, what=""):
    assert_density(got_density, ref, what)
    if got_cross is not None:
        assert_cross(got_density, got_cross, ref, what)
