"""Long-double reference of the overlap field's density per time origin, written from the definitions of include/ta_hip.h
(ta_overlap_density) and independent of the library:

    r2[t0, n]        = sum_d (x[t0 + tau, n, d] - x[t0, n, d])^2                     in long double
    a2[c]            = a_c a_c                                                        in float64
    phi_j[t0, n]     = sum_d k_j[d] x[t0, n, d]                                       in long double (the ORIGIN frame)
    W[j, c, l, t0]   = sum_{n: r2 < a2[c]} (cos, sin) phi_j[t0, n]  for t0 < T - tau_l, (0, 0) from there on   (K, C, L, T, 2)
    Q_e[c, l, t0]    = #{n: r2 < a2[c]}, the entry's exact count (overlap_ref.reference)

The inputs are scatter_ref.walk's random walks on a 1/1024 grid (exact in float32): every r2 is exact in float64 (asserted
by overlap_ref.reference), so the indicator is exact and only the phases and the sums carry rounding.  The cutoffs are
overlap_ref.CUTOFFS, the wavevectors scatter_ref.wavevectors' with an explicit k = 0 behind them.

The bar on either component of an entry, with u_r = 2^-53 and U = scatter_ref.unit_scale (max |k . x| / 2 pi of the call):

    Q_e (2 pi (D + 2) u_r U + (8 + Q_e) u_r)

which is partial_ref.density_bar with unit weights and no product rounding: per term the phase's 2 pi (D + 2) u_r U (D
roundings of u at scale U, the reduction is exact, the 2 pi scaling of what is left of it) and 8 u_r of the sine and cosine
themselves; the sum of Q_e terms of modulus <= 1 in any order adds at most Q_e u_r per term.  An entry nobody is inside of
(Q_e = 0) has bar 0: it must be exactly zero.

case() asserts what the cases are chosen for: for every case of 65 frames or more at least one (k != 0, cutoff, lag) whose W
varies over the origins with 0 < Q_e < N somewhere -- no test can pass on all-zero or all-N data alone."""
import functools

import numpy as np

import overlap_ref
import scatter_ref
from vanhove_ref import lag_sample

LD = np.longdouble
U_R = 2.0 ** -53
CUTOFFS = overlap_ref.CUTOFFS


def wavevectors(K, D, seed=1):
    """scatter_ref.wavevectors(K - 1, D, seed) with k = 0 behind them"""
    k = np.zeros((K, D))
    if K > 1:
        k[:K - 1] = scatter_ref.wavevectors(K - 1, D, seed)
    return k


def reference(x, k, lags, cutoffs):
    """(W (K, C, L, T, 2) long double, Q_e (C, L, T) int64)"""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    Q, _ = overlap_ref.reference(x, lags, cutoffs)
    a2 = np.asarray(cutoffs, dtype=np.float64) * np.asarray(cutoffs, dtype=np.float64)
    ph = scatter_ref.phases(x, k)  # (K, T, A)
    cs = np.stack([np.cos(ph), np.sin(ph)], axis=3)  # (K, T, A, 2)
    xl = x.astype(LD)
    W = np.zeros((len(k), len(a2), len(lags), T, 2), dtype=LD)
    for i, tau in enumerate(int(t) for t in lags):
        d = xl[tau:] - xl[:T - tau]
        r2 = (d * d).sum(axis=2).astype(np.float64)  # (exact: overlap_ref.reference has asserted it)
        for c, e in enumerate(a2):
            inside = (r2 < e).astype(LD)  # (T - tau, A)
            W[:, c, i, :T - tau] = np.einsum("ktnh,tn->kth", cs[:, :T - tau], inside)
            assert np.array_equal(inside.sum(axis=1).astype(np.int64), Q[c, i, :T - tau])
    return W, Q


def bar(x, k, Q):
    """(C, L, T) the bound on either component of W[:, c, l, t0]"""
    D = np.shape(x)[2]
    Qf = Q.astype(np.float64)
    return Qf * (2 * np.pi * (D + 2) * U_R * scatter_ref.unit_scale(x, k) + (8 + Qf) * U_R)


def non_trivial(W, Q, k, lags, n_particles):
    """the (k != 0, cutoff, lag) triples whose W varies over the valid origins with 0 < Q_e < N somewhere"""
    T = Q.shape[2]
    n = 0
    for j in range(len(k)):
        if not np.any(k[j]):
            continue
        for i, tau in enumerate(int(t) for t in lags):
            w, q = W[j, :, i, :T - tau], Q[:, i, :T - tau]
            if w.shape[1] < 2:
                continue
            varies = np.any(np.abs(w - w[:, :1]) > 1e-6, axis=(1, 2))
            partial = np.any((q > 0) & (q < n_particles), axis=1)
            n += int(np.count_nonzero(varies & partial))
    return n


@functools.lru_cache(maxsize=64)
def case(T, A, D, K=5, seed=1, cutoffs=CUTOFFS):
    """(x float64 (exact in float32), k, lags, W, Q, bar): computed once and shared; not to be modified"""
    x = scatter_ref.walk(T, A, D, seed)
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    k = wavevectors(K, D, seed)
    lags = lag_sample(T)
    W, Q = reference(x, k, lags, cutoffs)
    if T >= 65:
        assert non_trivial(W, Q, k, lags, A) >= 1, "W is constant over the origins, or Q_e is 0 or N, at every (k, cutoff, lag)"
    b = bar(x, k, Q)
    for a in (x, k, lags, W, Q, b):
        a.setflags(write=False)
    return x, k, lags, W, Q, b


def as_parts(w):
    """a call's W as float64 (K, C, L, T, 2): complex128 (K, C, L, T) from the host-facing calls, or already in parts"""
    w = np.asarray(w)
    if np.iscomplexobj(w):
        return np.ascontiguousarray(w).view(np.float64).reshape(w.shape + (2,))
    return w


def assert_w(got, ref, what="", pick=None, extra_bar=0.0):
    """A call's W against case(...)'s reference (pick: (wavevector indices, cutoff indices, lag indices) of the call within
    the case): every component within its entry's bar (+ extra_bar), an entry with Q_e = 0 exactly zero, +0.0 -- the sign
    bit too -- at t0 >= T - lag; the worst error / bar printed before it is asserted."""
    x, k, lags, W, Q, b = ref
    if pick is not None:
        js, cs, ls = (np.asarray(p) for p in pick)
        W, Q, b, lags = W[np.ix_(js, cs, ls)], Q[np.ix_(cs, ls)], b[np.ix_(cs, ls)], lags[ls]
    got = as_parts(got)
    assert got.dtype == np.float64 and got.shape == W.shape, (got.dtype, got.shape, W.shape)
    err = np.max(np.abs(got.astype(LD) - W), axis=4).astype(np.float64)  # (K, C, L, T)
    lim = b[None] + extra_bar * (Q[None] > 0)
    ratio = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), 0.0)))
    print(f"    {what} W: worst error / bar {ratio:.3f} (largest bar {float(b.max()):.3e}, largest |W| {float(np.max(np.abs(W))):.3e})")
    assert np.all(err <= lim), (what, np.argwhere(err > lim)[:5], float(err.max()))
    T = W.shape[3]
    for i, tau in enumerate(int(t) for t in lags):
        tail = got[:, :, i, T - tau:]
        assert not tail.any() and not np.signbit(tail).any(), (what, "entries past the last origin of lag", tau)
