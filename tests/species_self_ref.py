"""Reference for the per-species self terms: sum_{n in s} w_n^2 MSD_n(k) difference first, and sum_{n in s} w_n^2 VACF_n(k)
as direct sums, at chosen lags.  Nothing here knows about sorting, transforms or S1 - 2 S2.

Every term -- w (x[t+k] - x[t]) squared, or (w v[t]) (w v[t+k]) -- is formed in float64 from float64 inputs (three correctly
rounded operations: 3.3e-16 of the term at worst) and the terms are ADDED in NumPy long double, over frames, atoms and
dimensions at once.  The MSD's terms are all positive, so the reference is within 4e-16 of its own value; the VACF's
terms have mixed signs, so its error is 4e-16 of mean_t sum |w v[t]| |w v[t+k]|, which is of the order of the lag-0
value = max_k |self_s(k)|, the scale the tests' 1e-10 bar is relative to: five orders of magnitude below the bar.  Lags
run on a few threads, as oracle.numpy_oracle's per-lag forms do."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from current_ref import species_velocities
from onsager_ref import species_walk
from oracle import numpy_oracle as orc

LD = np.longdouble
SELF_MSD, SELF_VACF = 0, 1


def self_at_lags(y, lab, w, S, quantity, lags):
    """(S, len(lags)) float64: sum_{n: lab[n] = s} w_n^2 f_n(k) at each lag k of `lags`; f_n the per-atom MSD (SELF_MSD,
    lag 0 exactly 0) or VACF (SELF_VACF) of y (T, A, D); w None: all 1.  A species without atoms: zeros."""
    y = np.asarray(y, dtype=np.float64)
    T, A, D = y.shape
    w = np.ones(A) if w is None else np.asarray(w, dtype=np.float64)
    lab = np.asarray(lab)
    lags = [int(k) for k in lags]
    out = np.zeros((S, len(lags)))
    n_threads = max(1, min(8, os.cpu_count() or 1))
    for s in range(S):
        sel = np.flatnonzero(lab == s)
        if not sel.size:
            continue
        ys = np.ascontiguousarray(y[:, sel, :] * w[sel][None, :, None]).reshape(T, -1)

        def one(i, ys=ys, s=s):
            k = lags[i]
            if quantity == SELF_MSD:
                if k == 0:
                    return
                d = ys[k:] - ys[:T - k]
                terms = d * d
            else:
                terms = ys[:T - k] * ys[k:]
            out[s, i] = float(terms.sum(dtype=LD) / LD(T - k))

        with ThreadPoolExecutor(n_threads) as ex:
            list(ex.map(one, range(len(lags))))
    return out


def assert_self(got, want, lags, tol=1e-10, what=""):
    """every species within tol of max_k |self_s(k)| (conftest.scale_rel_err per species); a species whose reference is
    identically zero (no atoms) must be exactly zero.  Prints the worst figure before it asserts."""
    got = np.asarray(got)
    assert got.shape[0] == want.shape[0], (got.shape, want.shape)
    worst = 0.0
    for s in range(want.shape[0]):
        scale = float(np.abs(want[s]).max())
        err = float(np.abs(got[s][lags] - want[s]).max())
        if scale == 0.0:
            assert not got[s].any(), f"{what}: species {s} has no atoms: its row must be exactly zero"
            continue
        worst = max(worst, err / scale)
    print(f"    self {what}: worst species error {worst:.3e} of max_k |self_s(k)|")
    assert worst <= tol, f"{what}: {worst:.3e} of max_k |self_s(k)|"


def self_inputs(T, A, D, S, labels, quantity, seed=None):
    """(y, lab, w): species_walk (SELF_MSD) or species_velocities (SELF_VACF) rounded to float32 first, so that a float64
    and a float32 slab hold the same values; labels "rand": the generator's random order with unequal sizes, "alt":
    species n % S atom by atom (with D = 3 every straddling column pair holds two species)."""
    seed = T + A + S + D if seed is None else seed
    make = species_walk if quantity == SELF_MSD else species_velocities
    y, lab, w = make(T, A, S, seed=seed, D=D)
    y = y.astype(np.float32).astype(np.float64)
    if labels == "alt":
        lab = (np.arange(A) % S).astype(np.int32)
    return y, lab, w


@functools.lru_cache(maxsize=4)
def self_case(T, A, D, S, labels, quantity):
    """self_inputs(...) with its reference at orc.lag_sample(T): (y, lab, w, lags, want (S, len(lags))), read-only"""
    y, lab, w = self_inputs(T, A, D, S, labels, quantity)
    lags = orc.lag_sample(T)
    want = self_at_lags(y, lab, w, S, quantity, lags)
    for a in (y, lab, w, lags, want):
        a.setflags(write=False)
    return y, lab, w, lags, want
