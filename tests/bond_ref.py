"""Reference of the bond lifetime sums, written from the definitions of include/ta_hip.h (ta_bond_lifetime) and independent of
the library.  A bond is a row of 2 items (p, q) or of 3 (d, h, a) = donor, hydrogen, acceptor; per frame, in long double,

    r2         = |image(x_last - x_first)|^2                                  the box of frame t, as pair_ref
    u, v       = image(x_d - x_h), image(x_a - x_h)                           (triplets)
    ang_ok(c2) = u.v <= 0 and (u.v)^2 >= c2 (u.u) (v.v)                       INCLUSIVE; c2 = cos_cut^2
    form       = r2 < r_cut^2 and ang_ok(c2);  brk = r2 < r_break^2 and ang_ok(cb2)      the distance STRICT
    s(t)       = 2 if form, else 1 if brk, else 0                             (form implies brk)
    h(t)       = s(t) == 2 or (s(t) >= 1 and h(t - 1)),  h(-1) = 0            by a loop over the frames
    g(t)       = h(t) or (t1 < t < t2 with h(t1) = h(t2) = 1, t2 - t1 - 1 <= gap)      by a loop over the frames

and ci, runs, nb, cc are pair_ref.sums of g.  The inputs are random walks on a 1/32 grid in dyadic boxes of at most 8, the
cutoffs and cos_cut = -1/2, cos_break = -1/4 are dyadic: every step, (u.v)^2 and c2 (u.u) (v.v) included, is exact in float64
(asserted), so the comparisons are for EQUALITY and triplets exactly on the angle test the inclusive >=.  With a c2 that is
not dyadic (150 degrees) the reference is evaluated with the SAME float64 c2 and asserts that no triplet-frame lies within
1e-9 (u.u) (v.v) of the boundary, where the library's rounded products could decide differently."""
import functools

import numpy as np

from pair_ref import sums  # noqa: F401
from vanhove_distinct_ref import AXES, LD, dimensions, exact64

BOX = (8.0, 4.0, 8.0)
FRAME_BOXES = [(8.0, 4.0, 8.0), (8.0, 8.0, 4.0), (4.0, 4.0, 8.0), (4.0, 8.0, 4.0)]
R_CUT, R_BREAK = 1.5, 2.0  # dyadic; R_BREAK is half of the shortest box length
COS_CUT, COS_BREAK = -0.5, -0.25  # 120 and about 104.5 degrees
#: pattern_positions' distances of levels 2, 1, 0 and the cutoffs that go with them: exact in float32
LEVEL_DISTANCE = {2: 0.25, 1: 0.625, 0: 0.875}
PATTERN_CUTS = dict(r_cut=0.5, r_break=0.75)


def image(d, box, T, D, exact=True):
    if box is None:
        return d
    box = np.broadcast_to(np.asarray(box, dtype=np.float64), (T, D))
    assert np.all(np.frexp(box)[0] == 0.5) and box.max() <= 8.0, "the box lengths must be powers of two, at most 8"
    H = box[:, None, :].astype(LD)
    if not exact:
        return d - np.rint(d / H) * H
    sc = exact64(d / H, "d M")
    return exact64(d - np.rint(sc).astype(LD) * H, "the image").astype(LD)


def levels(x, bonds, box, r_cut, r_break, c2=None, cb2=None, margin=None):
    """s (P, T) in {0, 1, 2}.  x (T, A, D); bonds (P, 2) or (P, 3); box: None, (D,) or (T, D); c2, cb2: the SQUARED cosines as
    float64 (triplets).  margin None: every product must be exact in float64; else no triplet-frame may lie within margin
    (u.u) (v.v) of either angle boundary (nor within margin r^2 of a cutoff), and nothing else is asserted exact"""
    x = np.asarray(x, dtype=LD)
    T, A, D = x.shape
    bonds = np.asarray(bonds)
    n_at = bonds.shape[1]
    exact = margin is None
    d = image(x[:, bonds[:, -1], :] - x[:, bonds[:, 0], :], box, T, D, exact)  # (T, P, D)
    r2 = (d * d).sum(axis=2)
    rc2, rb2 = LD(np.float64(r_cut) * np.float64(r_cut)), LD(np.float64(r_break) * np.float64(r_break))
    if exact:
        exact64(r2, "r2")
    else:
        assert np.all(np.abs(r2 - rc2) > LD(margin) * rc2) and np.all(np.abs(r2 - rb2) > LD(margin) * rb2), "a frame lies on a cutoff"
    form, brk = r2 < rc2, r2 < rb2
    if n_at == 3:
        u = image(x[:, bonds[:, 0], :] - x[:, bonds[:, 1], :], box, T, D, exact)
        v = image(x[:, bonds[:, 2], :] - x[:, bonds[:, 1], :], box, T, D, exact)
        dot, uu, vv = (u * v).sum(axis=2), (u * u).sum(axis=2), (v * v).sum(axis=2)
        for c, name in ((c2, "c2"), (cb2, "cb2")):
            dd, rhs = dot * dot, LD(c) * uu * vv
            if exact:
                exact64(dd, "dot^2"), exact64(rhs, name + " uu vv")
            else:
                assert np.all(np.abs(dd - rhs) > LD(margin) * uu * vv), f"a triplet-frame lies on the {name} boundary"
            ok = (dot <= 0) & (dd >= rhs)
            if name == "c2":
                form = form & ok
            else:
                brk = brk & ok
    assert not np.any(form & ~brk), "form must imply brk"
    return np.ascontiguousarray(np.where(brk, np.where(form, 2, 1), 0).T)


def hysteresis(s):
    """h (P, T) bool by the loop of the definition"""
    h = np.zeros(s.shape, dtype=bool)
    for n, row in enumerate(s):
        on = False
        for t, level in enumerate(row):
            on = level == 2 or (level >= 1 and on)
            h[n, t] = on
    return h


def close_gaps(h, gap):
    """g (P, T) bool: every frame between two bonded frames t1 < t2 with t2 - t1 - 1 <= gap is bonded (t1, t2 the nearest
    bonded frames on either side, found by one loop forwards and one backwards)"""
    g = h.copy()
    P, T = h.shape
    for n in range(P):
        before, behind = np.full(T, -1), np.full(T, -1)
        last = -1
        for t in range(T):
            before[t] = last
            if h[n, t]:
                last = t
        last = -1
        for t in range(T - 1, -1, -1):
            behind[t] = last
            if h[n, t]:
                last = t
        for t in range(T):
            if not h[n, t] and before[t] >= 0 and behind[t] >= 0 and behind[t] - before[t] - 1 <= gap:
                g[n, t] = True
    return g


def filtered(s, gap):
    return close_gaps(hysteresis(np.asarray(s)), gap)


def walk32(T, A, D, seed, step=0.2, spread=6.0):
    """a random walk on a 1/32 grid, left unwrapped; exact in float32"""
    rng = np.random.default_rng(seed)
    steps = np.rint(rng.normal(scale=step * 32, size=(T, A, D)))
    start = np.rint(rng.uniform(0, spread, size=(1, A, D)) * 32)
    x = (np.cumsum(steps, axis=0) + start) / 32.0
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    return x


def boundary_triplets():
    """x (1, 12, 3) and bonds (4, 3) with the hydrogen at the origin of each triplet:
    u = (1, 1, 0), v = (-1, 0, 1): cos = -1/2 exactly (on cos_cut: bonded, the inclusive >=);  u = (1, 1, 0), v = (-1, 1, 1)
    (scaled by 1/2 like all four): cos = 0 (a right angle: dot = 0 satisfies dot <= 0, not cos_break);  u = (1, 0, 0), v = (-1, 0, 0): 180 degrees;
    u = (2, 2, 0) / 2, v = (-1, 0, 1) / 2 with |d - a| = sqrt(14) / 2 > r_cut: the angle holds, the distance decides"""
    rows = [((1, 1, 0), (-1, 0, 1), 0.5), ((1, 1, 0), (-1, 1, 1), 0.5), ((1, 0, 0), (-1, 0, 0), 0.5), ((2, 2, 0), (-1, 0, 1), 0.5)]
    x = np.zeros((1, 12, 3))
    for n, (u, v, scale) in enumerate(rows):
        origin = np.array([8.0 * n, 1.0, 2.0])
        x[0, 3 * n] = origin + scale * np.array(u)
        x[0, 3 * n + 1] = origin
        x[0, 3 * n + 2] = origin + scale * np.array(v)
    return x, np.arange(12, dtype=np.int32).reshape(4, 3)


@functools.lru_cache(maxsize=None)
def case(T, A, D, n_at, boxed, gap, seed=1, P=None):
    """(x, bonds, dims or None, axes, s, (ci, runs, nb, cc)) of a walk with R_CUT, R_BREAK, COS_CUT, COS_BREAK and `gap`: computed
    once and shared; not to be modified.  bonds: P (default 4 A) rows of distinct random items; boxed as pair_ref.case's"""
    x = walk32(T, A, D, seed)
    rng = np.random.default_rng(seed + 77)
    bonds = np.stack([rng.permutation(A)[:n_at] for _ in range(4 * A if P is None else P)]).astype(np.int32)
    axes = AXES[D]
    dims = box = None
    if boxed:
        dims = dimensions(FRAME_BOXES if boxed == "frames" else BOX, T)
        box = dims[:, list(axes)]
    s = levels(x, bonds, box, R_CUT, R_BREAK, COS_CUT * COS_CUT, COS_BREAK * COS_BREAK)
    for a in (x, bonds, s):
        a.setflags(write=False)
    return x, bonds, dims, axes, s, sums(filtered(s, gap))


def boundary_pairs():
    """x (1, 6, 3) and bonds (3, 2): partners at exactly R_CUT (level 1: the strict <), at exactly R_BREAK (level 0) and at
    R_CUT - 1/32 (level 2)"""
    x = np.zeros((1, 6, 3))
    x[0, :, 1] = 8.0 * (np.arange(6) // 2)
    x[0, 1, 0], x[0, 3, 2], x[0, 5, 0] = R_CUT, R_BREAK, R_CUT - 1.0 / 32
    return x, np.arange(6, dtype=np.int32).reshape(3, 2)


def constructed_levels(T, gap):
    """level rows (n, T) int8 that reach the filters' branches (clipped to the T frames there are): absences of exactly gap
    (filled) and gap + 1 frames (not filled) inside a word, across the 63|64 and across the 1023|1024 edge; a 63-frame absence
    from frame 40 on; leading and trailing absences; alternating; one level 2 followed by level 1 through three whole words;
    level 1 before the first 2; a 0 inside; level 1 only; 2 at frame 63 and 1 at 64; two hysteresis runs that the closing
    joins (the absence between them holds level-1 frames that hysteresis leaves unbonded)"""
    rows = []

    def new():
        rows.append(np.zeros(T, dtype=np.int8))
        return rows[-1]

    def put(r, lo, hi, level=2):
        r[max(lo, 0):max(min(hi, T - 1) + 1, 0)] = level

    for first_absent in (5, 62, 1022):
        for width in (gap, gap + 1):
            r = new()
            put(r, first_absent - 3, first_absent - 1)
            put(r, first_absent + width, first_absent + width + 2)
    r = new()
    put(r, 37, 39), put(r, 40 + 63, 40 + 65)
    put(new(), T // 3, T // 3 + 1)
    new()[::2] = 2
    r = new()
    put(r, 3, 3), put(r, 4, 4 + 3 * 64 + 10, 1)
    r = new()
    put(r, 0, 9, 1), put(r, 10, 10), put(r, 11, 20, 1)
    r = new()
    put(r, 2, 2), put(r, 3, 30, 1), put(r, 15, 15, 0)
    new()[:] = 1
    r = new()
    put(r, 63, 63), put(r, 64, 64, 1)
    r = new()
    put(r, 70, 70), put(r, 71, 71, 1), put(r, 73, 71 + gap, 1), put(r, 72 + gap, 72 + gap), put(r, 73 + gap, 73 + gap, 1)
    return np.stack(rows)


def pattern_positions(levels_, D=3):
    """x (T, 2 P, D) that realises the level patterns levels_ (P, T) over {0, 1, 2} with PATTERN_CUTS and no box: bond n is the
    atoms (2 n, 2 n + 1), atom 2 n rests at 4 n on the first axis and its partner sits LEVEL_DISTANCE[level] from it"""
    lv = np.asarray(levels_)
    P, T = lv.shape
    dist = np.select([lv == 2, lv == 1], [LEVEL_DISTANCE[2], LEVEL_DISTANCE[1]], LEVEL_DISTANCE[0])
    x = np.zeros((T, 2 * P, D))
    x[:, 0::2, 0] = 4.0 * np.arange(P)[None, :]
    x[:, 1::2, 0] = x[:, 0::2, 0] + dist.T
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    return x, np.arange(2 * P, dtype=np.int32).reshape(P, 2)
