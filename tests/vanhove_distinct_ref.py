"""Reference of the distinct van Hove histogram, written from the definitions of include/ta_hip.h (ta_vanhove_distinct) and
independent of the library:

    origins        t = stride o; lag tau uses those with t + tau < T
    d[p, q, :]     = x[t + tau, b_q, :] - x[t, a_p, :]                        in long double
    periodic axis: d -= rint(d / H) H                                         (H the box length of the ORIGIN frame)
    r2             = sum_j d_j^2
    e[b]           = (b dr)^2, b = 0 ... B                                    in float64
    bin            = searchsorted(e, r2, side="right") - 1, clipped to B     (B: the overflow bin)
    counts[l, bin] += 1 for every ordered pair with a_p != b_q               int64 (L, B + 1)

The inputs are scatter_ref.walk's random walks on a 1/1024 grid, left unwrapped (the coordinates run far outside the box),
and the box lengths are DYADIC: d / H is a scaling by a power of two, rint of it a whole number, d - k H a multiple of
2^-10 again and r2 a multiple of 2^-20 far below 2^53 of them -- every step is exact in float64, the reference asserts it,
and the counts are compared for EQUALITY."""
import functools

import numpy as np

from scatter_ref import walk

LD = np.longdouble

#: (n_bins, dr): a dyadic width (many pairs sit exactly on an edge; r_max = 1 is exactly half the shortest box) and a rounded one
BINS = [(64, 1.0 / 64), (50, 0.01)]
#: box lengths by axis (dyadic), and per-frame ones (cycled over the frames; the shortest analysed length stays 2)
BOX = (4.0, 2.0, 8.0)
FRAME_BOXES = [(4.0, 2.0, 8.0), (8.0, 4.0, 4.0), (2.0, 2.0, 16.0), (4.0, 8.0, 2.0)]
#: the box axis of each staged column, by D
AXES = {1: (1,), 2: (0, 2), 3: (0, 1, 2)}


def edges(n_bins, dr):
    return (np.arange(n_bins + 1, dtype=np.float64) * np.float64(dr)) ** 2


def exact64(v, what):
    v64 = v.astype(np.float64)
    assert np.array_equal(v64.astype(LD), v), f"{what} is not exact in float64: the counts would not be exact"
    return v64


def n_origins(T, lags, stride):
    return np.array([-(-(T - int(tau)) // stride) for tau in lags], dtype=np.int64)


def reference(x, lags, stride, a, b, box, n_bins, dr):
    """counts (L, B + 1) int64.  a, b: index arrays (None: all items / b = a); box: None, (D,) lengths of the staged columns
    or (T, D) per-frame ones"""
    return references(x, lags, stride, a, b, box, [(n_bins, dr)])[0]


def references(x, lags, stride, a, b, box, binnings):
    """reference() for several (n_bins, dr) at once: the squared distances are formed once"""
    x = np.asarray(x, dtype=LD)
    T, A, D = x.shape
    a = np.arange(A) if a is None else np.asarray(a)
    b = a if b is None else np.asarray(b)
    differ = a[:, None] != b[None, :]
    es = [edges(*bins) for bins in binnings]
    out = [np.zeros((len(lags), n_bins + 1), dtype=np.int64) for n_bins, _ in binnings]
    if box is not None:
        box = np.broadcast_to(np.asarray(box, dtype=np.float64), (T, D))
        assert np.all(np.frexp(box)[0] == 0.5), "the box lengths must be powers of two"
    per = max(1, (1 << 19) // (a.size * b.size))  # origins per numpy block
    for i, tau in enumerate(int(t) for t in lags):
        origins = np.arange(0, T - tau, stride)
        for k in range(0, origins.size, per):
            t0 = origins[k:k + per]
            d = x[t0 + tau][:, None, b, :] - x[t0][:, a, None, :]  # (origins, Na, Nb, D)
            if box is not None:
                H = box[t0][:, None, None, :].astype(LD)
                sc = exact64(d / H, "d M")
                d = d - np.rint(sc).astype(LD) * H
                exact64(d, "the image")
            r2 = exact64((d * d).sum(axis=3)[:, differ].ravel(), "r2")
            for counts, e, (n_bins, _) in zip(out, es, binnings):
                counts[i] += np.bincount(np.minimum(np.searchsorted(e, r2, side="right") - 1, n_bins), minlength=n_bins + 1)
    for counts in out:
        assert np.array_equal(counts.sum(axis=1), n_origins(T, lags, stride) * int(differ.sum()))
    return out


def lag_sample(T):
    """0, 1, 2, T // 2, T - 1 (those below T): odd and even"""
    return np.array(sorted(k for k in {0, 1, 2, T // 2, T - 1} if 0 <= k < T), dtype=np.int64)


def index_lists(kind, A):
    """(a, b) of one of the three relations of the two lists; None: all items / b = a"""
    if kind == "same":
        return None, None
    if kind == "disjoint":  # (one item: the same one on both sides)
        return (np.arange(0, A, 2), np.arange(1, A, 2)) if A > 1 else (np.arange(1), np.arange(1))
    assert kind == "overlap"
    return np.arange(0, max(1, (2 * A + 2) // 3)), np.arange(A // 3, A)


def dimensions(box, T):
    """the (T, 6) array ta_vanhove_distinct takes, of (3,) lengths or a list of them cycled over the frames"""
    rows = [box] * T if np.ndim(box) == 1 else [box[t % len(box)] for t in range(T)]
    return np.array([[*r, 90.0, 90.0, 90.0] for r in rows], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def positions(T, A, D, seed=1):
    x = walk(T, A, D, seed)
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def case(T, A, D, stride, kind, boxed, lags=None, seed=1):
    """(x float64 (exact in float32), lags, a, b, dims or None, axes, {(n_bins, dr): counts}): computed once and shared; not
    to be modified.  boxed: False, True (the constant BOX) or "frames" (FRAME_BOXES; lag 0 only)"""
    x = positions(T, A, D, seed)
    lags = (np.zeros(1, dtype=np.int64) if boxed == "frames" else lag_sample(T)) if lags is None else np.array(lags, dtype=np.int64)
    a, b = index_lists(kind, A)
    axes = AXES[D]
    dims = box = None
    if boxed:
        dims = dimensions(FRAME_BOXES if boxed == "frames" else BOX, T)
        box = dims[:, list(axes)]
    refs = dict(zip(BINS, references(x, lags, stride, a, b, box, BINS)))
    for r in refs.values():
        r.setflags(write=False)
    lags.setflags(write=False)
    return x, lags, a, b, dims, axes, refs


def assert_counts(got, want, what=""):
    """A call's counts against reference(...): equal; the figure printed before it is asserted."""
    bad = int(np.count_nonzero(np.asarray(got) != want))
    print(f"    {what} counts: {bad} of {want.size} differ (pairs {int(want.sum())}, in range {int(want[:, :-1].sum())})")
    assert got.dtype == np.int64 and got.shape == want.shape
    assert bad == 0, (what, np.argwhere(np.asarray(got) != want)[:5])
