"""Reference of the self van Hove histogram, written from the definitions of include/ta_hip.h (ta_vanhove) and independent
of the library:

    r2[t, n]       = sum_d (x[t + tau, n, d] - x[t, n, d])^2                 in long double
    e[b]           = (b dr)^2, b = 0 ... B                                    in float64
    bin            = searchsorted(e, r2, side="right") - 1, clipped to B     (B: the overflow bin)
    counts[l, b]   = the pairs (t, n), t < T - tau_l, of bin b               int64 (L, B + 1)
    moments[l, :]  = (sum r2, sum r2 r2)                                     in long double

The inputs are scatter_ref.walk's random walks on a 1/1024 grid (exact in float32): every r2 is then an integer multiple of
2^-20 far below 2^53 of them, exact in float64, so the counts are exact integers and are compared for EQUALITY; the moments
within 1e-10 relative, the project's standing bar."""
import functools

import numpy as np

from scatter_ref import walk

LD = np.longdouble

#: (n_bins, dr): a dyadic width (many pairs sit exactly on an edge: the <= side) and a rounded one
BINS = [(64, 0.125), (50, 0.1)]


def lag_sample(T):
    """0, 1, 2, 3, 7, both sides of 64, 256 and a workgroup's 1024-frame tile, T/2, T - 2, T - 1 (those below T): odd and even"""
    want = {0, 1, 2, 3, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, T // 2, T - 2, T - 1}
    return np.array(sorted(k for k in want if 0 <= k < T), dtype=np.int64)


def edges(n_bins, dr):
    return (np.arange(n_bins + 1, dtype=np.float64) * np.float64(dr)) ** 2


def reference(x, lags, n_bins, dr):
    """(counts (L, B + 1) int64, moments (L, 2) long double)"""
    x = np.asarray(x, dtype=LD)
    T = x.shape[0]
    e = edges(n_bins, dr)
    counts = np.zeros((len(lags), n_bins + 1), dtype=np.int64)
    moments = np.zeros((len(lags), 2), dtype=LD)
    for i, tau in enumerate(int(t) for t in lags):
        d = x[tau:] - x[:T - tau]
        r2 = (d * d).sum(axis=2).ravel()
        r2_64 = r2.astype(np.float64)
        assert np.array_equal(r2_64.astype(LD), r2), "r2 is not exact in float64: the counts would not be exact"
        b = np.minimum(np.searchsorted(e, r2_64, side="right") - 1, n_bins)
        counts[i] = np.bincount(b, minlength=n_bins + 1)
        moments[i] = r2.sum(), (r2 * r2).sum()
    return counts, moments


@functools.lru_cache(maxsize=64)
def case(T, A, D, seed=1):
    """(x float64 (exact in float32), lags, {(n_bins, dr): (counts, moments)}): computed once and shared; not to be modified"""
    x = walk(T, A, D, seed)
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    lags = lag_sample(T)
    refs = {}
    for bins in BINS:
        refs[bins] = reference(x, lags, *bins)
        for a in refs[bins]:
            a.setflags(write=False)
    x.setflags(write=False)
    lags.setflags(write=False)
    return x, lags, refs


def assert_vanhove(got_counts, got_moments, want, what=""):
    """A call's outputs against reference(...): the counts equal, the moments within 1e-10 relative, each lag by its own value;
    every figure printed before it is asserted."""
    counts, moments = want
    if got_counts is not None:
        bad = int(np.count_nonzero(np.asarray(got_counts) != counts))
        print(f"    {what} counts: {bad} of {counts.size} differ (pairs {int(counts.sum())})")
        assert got_counts.dtype == np.int64 and got_counts.shape == counts.shape
        assert bad == 0, (what, np.argwhere(np.asarray(got_counts) != counts)[:5])
    if got_moments is not None:
        got = np.asarray(got_moments, dtype=LD)
        scale = np.where(moments > 0, moments, LD(1))
        err = float(np.max(np.abs(got - moments) / scale))
        print(f"    {what} moments: {err:.3e} relative")
        assert err <= 1e-10, (what, err)
