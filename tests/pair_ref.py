"""Reference of the pair lifetime sums, written from the definitions of include/ta_hip.h (ta_pair_find, ta_pair_lifetime) and
independent of the library:

    d[p, q, :]   = x[t, q, :] - x[t, p, :]                                   in long double
    periodic:    d -= rint(d / H(t)) H(t)                                     (the box of frame t: both items at the SAME frame)
    h_pq(t)      = sum_j d_j^2 < r_cut^2                                      (strictly below)
    found        = {(a_p, b_q): a_p != b_q, h = 1 in a frame t = stride o}    sorted; b = a: only a_p < b_q
    ci[tau]      = sum_pairs sum_{t < T - tau} h(t) h(t + tau)               by the double loop
    runs[l]      = the maximal runs of exactly l consecutive bonded frames    by scanning each series
    nb[t]        = sum_pairs h(t)
    cc[tau]      = sum_l max(0, l - tau) runs[l] = sum_pairs sum_{t < T - tau} prod_{s = t}^{t + tau} h(s): both, asserted equal

The inputs are scatter_ref.walk's random walks on a 1/1024 grid, the box lengths and r_cut are DYADIC: every step is exact in
float64 (asserted, with vanhove_distinct_ref's asserts), so every comparison is for EQUALITY, and pairs that sit exactly on
r2 == r_cut^2 test the strict <.  pattern_positions builds positions that realise a given bit pattern."""
import functools

import numpy as np

from vanhove_distinct_ref import AXES, BOX, FRAME_BOXES, LD, dimensions, exact64, positions  # noqa: F401

R_CUT = 1.0  # dyadic, half of the shortest box length of BOX and FRAME_BOXES


def indicator(x, pairs, box, r_cut):
    """h (P, T) bool of the atom pairs (P, 2) of x (T, A, D); box: None, (D,) lengths or (T, D) per-frame ones"""
    x = np.asarray(x, dtype=LD)
    T, A, D = x.shape
    pairs = np.asarray(pairs).reshape(-1, 2)
    rc2 = exact64(LD(r_cut) * LD(r_cut) * np.ones(1, dtype=LD), "r_cut^2")[0]
    d = x[:, pairs[:, 1], :] - x[:, pairs[:, 0], :]  # (T, P, D)
    if box is not None:
        box = np.broadcast_to(np.asarray(box, dtype=np.float64), (T, D))
        assert np.all(np.frexp(box)[0] == 0.5), "the box lengths must be powers of two"
        H = box[:, None, :].astype(LD)
        sc = exact64(d / H, "d M")
        d = d - np.rint(sc).astype(LD) * H
        exact64(d, "the image")
    r2 = exact64((d * d).sum(axis=2), "r2")
    return np.ascontiguousarray((r2 < rc2).T)


def all_pairs(a, b):
    """the pairs the search looks at: (a_p, b_q), a_p != b_q; b None: a_p < b_q"""
    a = np.asarray(a)
    if b is None:
        i, j = np.triu_indices(a.size, k=1)
        return np.stack([a[i], a[j]], axis=1)
    b = np.asarray(b)
    i, j = np.nonzero(a[:, None] != b[None, :])
    return np.stack([a[i], b[j]], axis=1)


def found(x, a, b, box, r_cut, stride):
    """the found list as a sorted (n, 2) array: bonded in at least one searched frame"""
    T, A, D = np.shape(x)
    a = np.arange(A) if a is None else np.asarray(a)
    cand = all_pairs(a, b)
    if cand.shape[0] == 0:
        return cand.reshape(0, 2)
    h = indicator(x, cand, box, r_cut)
    keep = cand[h[:, ::stride].any(axis=1)]
    return keep[np.lexsort((keep[:, 1], keep[:, 0]))]


def run_lengths(h):
    """runs (T + 1,) int64 by scanning each series"""
    P, T = h.shape
    runs = np.zeros(T + 1, dtype=np.int64)
    for series in h:
        n = 0
        for bit in series:
            if bit:
                n += 1
            elif n:
                runs[n] += 1
                n = 0
        if n:
            runs[n] += 1
    return runs


def sums(h):
    """(ci (T,), runs (T + 1,), nb (T,), cc (T,)) int64 of the indicator h (P, T)"""
    P, T = h.shape
    hi = h.astype(np.int64)
    ci = np.array([int((hi[:, :T - tau] * hi[:, tau:]).sum()) for tau in range(T)], dtype=np.int64)
    runs = run_lengths(h)
    nb = hi.sum(axis=0)
    ell = np.arange(T + 1)
    cc = np.array([int((np.maximum(0, ell - tau) * runs).sum()) for tau in range(T)], dtype=np.int64)
    # the per-origin definition: prod_{s = t}^{t + tau} h(s), built up lag by lag
    alive, direct = hi.copy(), np.zeros(T, dtype=np.int64)
    for tau in range(T):
        if tau:
            alive = alive[:, :T - tau] * hi[:, tau:]
        direct[tau] = alive.sum()
    assert np.array_equal(cc, direct), "the run-length form of the continuous sum differs from its definition"
    assert int((ell * runs).sum()) == int(nb.sum())
    return ci, runs, nb, cc


def correlations(ci, nb, cc):
    """(intermittent, continuous) = (ci, cc) / n0, n0[tau] = sum_{t < T - tau} nb[t]: one float64 division of exact integers"""
    n0 = np.cumsum(nb)[::-1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return ci.astype(np.float64) / n0, cc.astype(np.float64) / n0


@functools.lru_cache(maxsize=None)
def case(T, A, D, kind, boxed, stride=1, seed=1):
    """(x, a, b, dims or None, axes, pairs, (ci, runs, nb, cc)) of a walk: computed once and shared; not to be modified.
    kind: "same", "disjoint" or "explicit" (every third pair of the disjoint search, in reverse order); boxed: False, True (the
    constant BOX) or "frames" (FRAME_BOXES)"""
    x = positions(T, A, D, seed)
    axes = AXES[D]
    dims = box = None
    if boxed:
        dims = dimensions(FRAME_BOXES if boxed == "frames" else BOX, T)
        box = dims[:, list(axes)]
    a, b = (None, None) if kind == "same" else (np.arange(0, A, 2), np.arange(1, A, 2))
    pairs = found(x, a, b, box, R_CUT, stride)
    if kind == "explicit":
        pairs = np.ascontiguousarray(all_pairs(a, b)[::3][::-1])
    out = sums(indicator(x, pairs, box, R_CUT)) if pairs.shape[0] else None
    return x, a, b, dims, axes, pairs, out


def pattern_positions(bits, D=3):
    """x (T, 2 P, D) that realises the bit patterns bits (P, T) with r_cut = 0.5 and no box: pair n is the atoms (2 n, 2 n + 1),
    atom 2 n rests at 4 n on the first axis and its partner sits 0.25 (bonded) or 0.75 (not bonded) from it.  Exact in float32."""
    bits = np.asarray(bits, dtype=bool)
    P, T = bits.shape
    x = np.zeros((T, 2 * P, D))
    x[:, 0::2, 0] = 4.0 * np.arange(P)[None, :]
    x[:, 1::2, 0] = x[:, 0::2, 0] + np.where(bits.T, 0.25, 0.75)
    return x, np.arange(2 * P, dtype=np.int32).reshape(P, 2)


def pattern(name, T):
    """one series (T,) bool: "always", "never", "alternating", or (lo, hi): a single run covering exactly frames [lo, hi]"""
    if name == "always":
        return np.ones(T, dtype=bool)
    if name == "never":
        return np.zeros(T, dtype=bool)
    if name == "alternating":
        return np.arange(T) % 2 == 0
    lo, hi = name
    return (np.arange(T) >= lo) & (np.arange(T) <= hi)
