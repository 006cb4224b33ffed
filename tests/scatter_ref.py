"""Long-double reference of the intermediate scattering functions, written from the definitions of include/ta_hip.h
(ta_scatter) and independent of the library:

    phi_j[t, n]    = sum_d k_j[d] x[t, n, d]
    self[j, tau]   = 1/(T - tau) sum_{t < T - tau} sum_n cos(phi_j[t + tau, n] - phi_j[t, n])
    density[j, t]  = (sum_n cos phi_j[t, n], sum_n sin phi_j[t, n])
    coll[j, tau]   = 1/(T - tau) sum_{t < T - tau} (rc[t] rc[t + tau] + rs[t] rs[t + tau])

x: the float64 values actually staged (for a float32 slab: rounded to float32 first, by the caller).  The lag sums are
direct sums at a given list of lags; cos(a - b) is formed as cos a cos b + sin a sin b from the long-double (cos, sin) of
the long-double phases, so a case costs one cos / sin per (wavevector, frame, atom) whatever the number of lags."""
import functools

import numpy as np

LD = np.longdouble
U_R = 2.0 ** -53


def lag_sample(T):
    """0, 1, 2, both sides of 64 and 512, T/2, T - 2, T - 1 (those below T)"""
    want = {0, 1, 2, 63, 64, 65, 511, 512, 513, T // 2, T - 2, T - 1}
    return np.array(sorted(k for k in want if 0 <= k < T), dtype=np.int64)


def phases(x, k):
    """(K, T, A) long-double phases"""
    return np.einsum("kd,tnd->ktn", np.asarray(k, dtype=LD), np.asarray(x, dtype=LD))


def unit_scale(x, k):
    """U = max |k . x| / (2 pi) over the call"""
    return float(np.max(np.abs(phases(x, k))) / (2 * LD(np.pi)))


def density_bar(x, k):
    """N (2 pi (D + 2) u_r U + 8 u_r): the bound on either density component (ta_hip.h)"""
    T, A, D = np.shape(x)
    return A * (2 * np.pi * (D + 2) * U_R * unit_scale(x, k) + 8 * U_R)


def acf_at(c, s, lags):
    """[..., len(lags)]: 1/(T - tau) sum_t (c[t] c[t + tau] + s[t] s[t + tau]) summed over every axis behind the time axis
    (axis 1 of (K, T, ...) long-double arrays)"""
    K, T = c.shape[:2]
    out = np.zeros((K, len(lags)), dtype=LD)
    for i, tau in enumerate(lags):
        n = T - int(tau)
        prod = c[:, :n] * c[:, int(tau):] + s[:, :n] * s[:, int(tau):]
        out[:, i] = prod.reshape(K, -1).sum(axis=1) / n
    return out


def reference(x, k, lags):
    """(self (K, len(lags)), density (K, T, 2), coll (K, len(lags))) in long double"""
    ph = phases(x, k)
    c, s = np.cos(ph), np.sin(ph)
    rho = np.stack([c.sum(axis=2), s.sum(axis=2)], axis=2)
    return acf_at(c, s, lags), rho, coll_at(rho, lags)


def coll_at(density, lags):
    """coll at `lags` of a (K, T, 2) density (e.g. the one a call returned), in long double"""
    rho = np.asarray(density, dtype=LD)
    return acf_at(rho[:, :, 0], rho[:, :, 1], lags)


def walk(T, A, D, seed, step=0.3, offset=50.0):
    """a random walk around `offset` on a 1/1024 grid: the values are exact in float32 while they stay below 2^13"""
    rng = np.random.default_rng(seed)
    steps = np.rint(rng.normal(scale=step * 1024, size=(T, A, D)))
    start = np.rint(rng.uniform(0, offset, size=(1, A, D)) * 1024)
    return (np.cumsum(steps, axis=0) + start) / 1024.0


def wavevectors(K, D, seed, kmax=6.0):
    """K wavevectors with components within +-kmax rad per length unit, the first along an axis"""
    rng = np.random.default_rng(seed + 1000)
    k = rng.uniform(-kmax, kmax, size=(K, D))
    k[0] = 0.0
    k[0, 0] = 1.25
    return k


@functools.lru_cache(maxsize=32)
def case(T, A, D, K, seed=1):
    """(x float64 (exact in float32), k, lags, self, density, bar): computed once and shared; not to be modified"""
    x, k = walk(T, A, D, seed), wavevectors(K, D, seed)
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    lags = lag_sample(T)
    fs, rho, _ = reference(x, k, lags)
    out = (x, k, lags, fs, rho, density_bar(x, k))
    for a in out[:5]:
        a.setflags(write=False)
    return out


def assert_scatter(got_self, got_density, got_coll, ref, what=""):
    """The three outputs of a call against case(...)'s reference: the density within its bar, self within 1e-10 of its max
    at the lags, coll within 1e-10 of its max against the long-double autocorrelation of the RETURNED density; every figure
    printed before it is asserted."""
    x, k, lags, fs, rho, bar = ref
    if got_density is not None:
        err = float(np.max(np.abs(np.asarray(got_density, dtype=LD) - rho)))
        print(f"    {what} density: {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (what, err, bar)
    if got_self is not None:
        scale = float(np.max(np.abs(fs)))
        err = float(np.max(np.abs(np.asarray(got_self, dtype=LD)[:, lags] - fs))) / scale
        print(f"    {what} self: {err:.3e} of {scale:.3e}")
        assert err <= 1e-10, (what, err)
    if got_coll is not None:
        want = coll_at(got_density, lags)
        scale = float(np.max(np.abs(want)))
        err = float(np.max(np.abs(np.asarray(got_coll, dtype=LD)[:, lags] - want))) / scale
        print(f"    {what} coll: {err:.3e} of {scale:.3e}")
        assert err <= 1e-10, (what, err)
