"""Reference of the shell residence sums, written from the definitions of include/ta_hip.h (ta_shell_residence) and independent
of the library.  Per observed item q of b and frame t, over ALL reference items p of a with another id,

    d        = x[t, q, :] - x[t, p, :];  periodic: d -= rint(d / H(t)) H(t)            the box of frame t
    form     = some p with |d|^2 < r_cut^2;  brk = some p with |d|^2 < r_break^2         both STRICT
    s_q(t)   = 2 if form, else 1 if brk, else 0
    h_q(t)   = s(t) == 2 or (s(t) >= 1 and h(t - 1)),  h(-1) = 0                         by a loop over the frames
    g_q(t)   = h(t) or (t1 < t < t2 with h(t1) = h(t2) = 1, t2 - t1 - 1 <= gap)          by a loop over the frames

and ci, runs, nb, cc are pair_ref.sums of g (runs by scanning each series; cc from the runs AND from the per-origin product,
asserted equal there).

All inputs lie on the grid of multiples of 2^-10, box lengths are powers of two and the cutoffs are dyadic.  The reference
works in INTEGER grid units (int64): every difference, image step and squared distance is then exact by construction, and it
asserts for every (p, q, t) that the float64 evaluation of the library is exact as well (the inputs are on the grid and
survive float32, d / H has a power-of-two divisor, and every r2 stays below 2^53 grid units squared).  So every comparison is
for EQUALITY, and items exactly on a cutoff test the strict <."""
import functools

import numpy as np

from pair_ref import sums  # noqa: F401
from vanhove_distinct_ref import AXES, BOX, FRAME_BOXES, dimensions

GRID = 1024
#: pattern_positions' distances of levels 2, 1, 0 from the owning reference item and the cutoffs that go with them
LEVEL_DISTANCE = {2: 0.25, 1: 0.625, 0: 0.875}
PATTERN_CUTS = dict(r_cut=0.5, r_break=0.75)
REF_SPACING = 8.0  # pattern_positions' reference items sit this far apart: an observed item is near its owner alone


def grid_units(v, what):
    """v as int64 multiples of 2^-10, asserted exact"""
    v = np.asarray(v, dtype=np.float64)
    i = np.rint(v * GRID).astype(np.int64)
    assert np.array_equal(i / GRID, v), f"{what} is not on the 2^-10 grid"
    return i


def levels(x, a, b, box, r_cut, r_break, chunk=1 << 22):
    """s (N_b, T) in {0, 1, 2}.  x (T, A, D); a, b: index arrays (None: all items / b = a); box: None, (D,) or (T, D)"""
    x = np.asarray(x, dtype=np.float64)
    T, A, D = x.shape
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64)), "float32 staging must be lossless"
    xi = grid_units(x, "a position")
    a = np.arange(A) if a is None else np.asarray(a)
    b = a if b is None else np.asarray(b)
    rc2, rb2 = int(grid_units(r_cut, "r_cut")) ** 2, int(grid_units(r_break, "r_break")) ** 2
    assert 0 < rc2 <= rb2
    Hi = None
    if box is not None:
        box = np.broadcast_to(np.asarray(box, dtype=np.float64), (T, D))
        assert np.all(np.frexp(box)[0] == 0.5), "the box lengths must be powers of two"
        Hi = grid_units(box, "a box length")
    other = b[:, None] != a[None, :]
    s = np.zeros((b.size, T), dtype=np.int8)
    step = max(1, chunk // max(1, a.size * b.size * D))
    for t0 in range(0, T, step):
        t1 = min(T, t0 + step)
        d = xi[t0:t1, b][:, :, None, :] - xi[t0:t1, a][:, None, :, :]  # (t, N_b, N_a, D)
        if Hi is not None:
            H = Hi[t0:t1, None, None, :]
            assert np.abs(d).max(initial=0) < 2 ** 52  # (d / H below: exact, H a power of two)
            d = d - np.rint(d / H).astype(np.int64) * H
        assert np.abs(d).max(initial=0) < 2 ** 25, "r2 would leave the exact range of float64"  # (3 d^2 < 2^53)
        r2 = (d * d).sum(axis=3)
        form = ((r2 < rc2) & other[None]).any(axis=2)
        brk = ((r2 < rb2) & other[None]).any(axis=2)
        s[:, t0:t1] = np.where(brk, np.where(form, 2, 1), 0).T
    return s


def hysteresis(s):
    """h (N, T) bool: the definition's recurrence, frame by frame"""
    s = np.asarray(s)
    h = np.zeros(s.shape, dtype=bool)
    on = np.zeros(s.shape[0], dtype=bool)
    for t in range(s.shape[1]):
        on = (s[:, t] == 2) | ((s[:, t] >= 1) & on)
        h[:, t] = on
    return h


def close_gaps(h, gap):
    """g (N, T) bool: a frame between the nearest inside frames t1 < t < t2 with t2 - t1 - 1 <= gap is inside"""
    N, T = h.shape
    before, behind = np.full((N, T), -1), np.full((N, T), -1)
    last = np.full(N, -1)
    for t in range(T):
        before[:, t] = last
        last = np.where(h[:, t], t, last)
    last = np.full(N, -1)
    for t in range(T - 1, -1, -1):
        behind[:, t] = last
        last = np.where(h[:, t], t, last)
    return h | ((before >= 0) & (behind >= 0) & (behind - before - 1 <= gap))


def filtered(s, gap):
    return close_gaps(hysteresis(s), gap)


def walk(T, A, D, seed, spread, step=0.125):
    """a random walk on the 2^-10 grid that starts inside a cube of side `spread`, left unwrapped; exact in float32"""
    rng = np.random.default_rng(seed)
    steps = np.rint(rng.normal(scale=step * GRID, size=(T, A, D)))
    start = np.rint(rng.uniform(0, spread, size=(1, A, D)) * GRID)
    return (np.cumsum(steps, axis=0) + start) / GRID


def ball(r, D):
    return {1: 2 * r, 2: np.pi * r * r, 3: 4.0 / 3.0 * np.pi * r ** 3}[D]


@functools.lru_cache(maxsize=None)
def case(T, Na, Nb, D, kind, boxed, gap, seed=1):
    """(x, a, b, dims or None, axes, cuts, s, (ci, runs, nb, cc)) of a walk: computed once and shared; not to be modified.
    kind "disjoint": Na reference and Nb observed items drawn from Na + Nb + 3 items (both lists sorted, interleaved);
    "same": one list of Nb items (Na is ignored: a = b = None, all items).  boxed: False, True (BOX) or "frames"
    (FRAME_BOXES).  cuts = dict(r_cut, r_break): dyadic, r_break at most 1 (half the shortest box length), sized so that
    about half of the observed items are inside."""
    rng = np.random.default_rng(seed + 1000)
    if kind == "same":
        A, a, b, n_ref = Nb, None, None, Nb
    else:
        A, n_ref = Na + Nb + 3, Na
        perm = rng.permutation(A)
        a, b = np.sort(perm[:Na]), np.sort(perm[Na:Na + Nb])
    axes = AXES[D]
    dims = box = None
    if boxed:
        dims = dimensions(FRAME_BOXES if boxed == "frames" else BOX, T)
        box = dims[:, list(axes)]
        volume = float(np.prod(box, axis=1).min())
        r_cut = next((r for r in (0.75, 0.5, 0.375, 0.25, 0.1875, 0.125, 2.0 ** -4, 2.0 ** -5, 2.0 ** -6, 2.0 ** -7)
                      if n_ref * ball(r, D) <= 0.7 * volume), 2.0 ** -8)
        spread = 8.0
    else:
        r_cut = 0.75
        spread = max(2.0, (n_ref * ball(r_cut, D) / 0.5) ** (1.0 / D))
    cuts = dict(r_cut=r_cut, r_break=r_cut * 1.25)
    x = walk(T, A, D, seed, spread)
    s = levels(x, a, b, box, **cuts)
    out = sums(filtered(s, gap))
    for v in (x, s):
        v.setflags(write=False)
    return x, a, b, dims, axes, cuts, s, out


def pattern_positions(levels_, owner=None, n_ref=1, D=3):
    """(x (T, n_ref + N, D), a, b) that realises the level patterns levels_ (N, T) over {0, 1, 2} with PATTERN_CUTS and no
    box: the reference items 0 ... n_ref - 1 rest REF_SPACING apart on the first axis, observed item n (index n_ref + n) sits
    LEVEL_DISTANCE[level] from reference item owner[n, t] (default: n mod n_ref): far from every other reference item"""
    lv = np.asarray(levels_)
    N, T = lv.shape
    own = np.broadcast_to(np.arange(N)[:, None] % n_ref if owner is None else np.asarray(owner), (N, T))
    dist = np.select([lv == 2, lv == 1], [LEVEL_DISTANCE[2], LEVEL_DISTANCE[1]], LEVEL_DISTANCE[0])
    x = np.zeros((T, n_ref + N, D))
    x[:, :n_ref, 0] = REF_SPACING * np.arange(n_ref)[None, :]
    x[:, n_ref:, 0] = (REF_SPACING * own + dist).T
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    return x, np.arange(n_ref), np.arange(n_ref, n_ref + N)
