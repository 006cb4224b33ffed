"""Reference of the self-overlap per time origin and of chi_4, written from the definitions of include/ta_hip.h (ta_overlap)
and independent of the library:

    r2[t0, n]      = sum_d (x[t0 + tau, n, d] - x[t0, n, d])^2               in long double
    a2[c]          = a_c a_c                                                  in float64
    Q[c, l, t0]    = #{n: r2 < a2[c]} for t0 < T - tau_l, 0 from there on    int64 (C, L, T)
    q[c, l]        = mean over t0 < T - tau_l of Q / N                        in long double
    chi4[c, l]     = the two-pass variance over the same origins of Q, / N   in long double; NaN with fewer than two origins

The inputs are scatter_ref.walk's random walks on a 1/1024 grid (exact in float32): every r2 is an integer multiple of 2^-20,
exact in float64 (asserted, as vanhove_ref does), so Q is an exact integer array and is compared for EQUALITY, no entry excluded.

The cutoffs: 0.5 sits ON the grid of r2 in one dimension (|d| = 512 steps: the strict side of the comparison decides
those pairs), 0.7 off every grid, 1.5 and 4.0 reach the longer lags.  case() asserts what the cases are chosen for: pairs
exactly on a = 0.5 in the D = 1 case, and for every case of 65 frames or more at least one (cutoff, lag) whose Q is neither
all 0 nor all N and varies over the origins -- no test can pass on all-zero or all-N data alone."""
import functools

import numpy as np

from scatter_ref import walk
from vanhove_ref import lag_sample

LD = np.longdouble

CUTOFFS = (0.5, 0.7, 1.5, 4.0)


def reference(x, lags, cutoffs):
    """(Q (C, L, T) int64, pairs exactly on a cutoff (C,))"""
    x = np.asarray(x, dtype=LD)
    T = x.shape[0]
    a2 = np.asarray(cutoffs, dtype=np.float64) * np.asarray(cutoffs, dtype=np.float64)
    Q = np.zeros((len(a2), len(lags), T), dtype=np.int64)
    on_edge = np.zeros(len(a2), dtype=np.int64)
    for i, tau in enumerate(int(t) for t in lags):
        d = x[tau:] - x[:T - tau]
        r2 = (d * d).sum(axis=2)
        r2_64 = r2.astype(np.float64)
        assert np.array_equal(r2_64.astype(LD), r2), "r2 is not exact in float64: Q would not be exact"
        for c, e in enumerate(a2):
            Q[c, i, :T - tau] = (r2_64 < e).sum(axis=1)
            on_edge[c] += int((r2_64 == e).sum())
    return Q, on_edge


def moments(Q, lags, n_particles):
    """(q, chi4), both (C, L) long double, from an exact Q"""
    C, L, T = Q.shape
    q, chi4 = np.zeros((C, L), dtype=LD), np.full((C, L), np.nan, dtype=LD)
    for i, tau in enumerate(int(t) for t in lags):
        v = Q[:, i, :T - tau].astype(LD)
        mean = v.sum(axis=1) / LD(T - tau)
        q[:, i] = mean / LD(n_particles)
        if T - tau >= 2:
            dev = v - mean[:, None]
            chi4[:, i] = (dev * dev).sum(axis=1) / LD(T - tau) / LD(n_particles)
    return q, chi4


def non_trivial(Q, lags, n_particles):
    """the (cutoff, lag) pairs whose Q over the valid origins is neither all 0 nor all N and varies"""
    C, L, T = Q.shape
    n = 0
    for i, tau in enumerate(int(t) for t in lags):
        v = Q[:, i, :T - tau]
        if v.shape[1]:
            n += int(np.count_nonzero((v.max(axis=1) > v.min(axis=1)) & ~np.all(v == 0, axis=1) & ~np.all(v == n_particles, axis=1)))
    return n


@functools.lru_cache(maxsize=64)
def case(T, A, D, seed=1, cutoffs=CUTOFFS):
    """(x float64 (exact in float32), lags, Q, q, chi4): computed once and shared; not to be modified"""
    x = walk(T, A, D, seed)
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    lags = lag_sample(T)
    Q, on_edge = reference(x, lags, cutoffs)
    if D == 1 and T >= 65 and 0.5 in cutoffs:
        assert on_edge[cutoffs.index(0.5)] > 0, "no pair exactly on a = 0.5: the strict side is not exercised"
    if T >= 65:
        assert non_trivial(Q, lags, A) >= 1, "Q is all 0, all N or constant over the origins at every (cutoff, lag)"
    q, chi4 = moments(Q, lags, A)
    for a in (x, lags, Q, q, chi4):
        a.setflags(write=False)
    return x, lags, Q, q, chi4


def assert_q(got, want, lags, what=""):
    """A call's Q against reference(...): equal, every entry; zeros at t0 >= T - lag; the figure printed before it is asserted"""
    got = np.asarray(got)
    assert got.dtype == np.int64 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    bad = int(np.count_nonzero(got != want))
    print(f"    {what} Q: {bad} of {want.size} differ (sum {int(want.sum())})")
    assert bad == 0, (what, np.argwhere(got != want)[:5])
    T = want.shape[2]
    for i, tau in enumerate(int(t) for t in lags):
        assert not got[:, i, T - tau:].any(), (what, "entries past the last origin of lag", tau)
