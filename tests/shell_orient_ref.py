"""Reference of the shell-resolved reorientation sums, written from the definitions of include/ta_hip.h (ta_shell_orient) and
independent of the library, on top of shell_ref.  A vector n is a row of 2 (bond) or 3 atoms; with d(a -> b) = x_b - x_a,
reduced by d -= rint(d / H(t)) H(t) where there is a box,

    bond: v = d(a -> b);   bisector: v = d(a -> b) + d(a -> c);   normal: v = d(a -> b) x d(a -> c);   u = v / |v|, 0 for v = 0

and with g (N_b, T) the shell series of the rows' anchor atoms, for tau = 0 ... L and c = u_n(t) . u_n(t + tau)

    S[tau, 0] = sum over (n, t) of w c,    S[tau, 1] = sum over (n, t) of w c^2,    N[tau] = sum over (n, t) of w

with shell_msd_ref's gates w.  The anchors are shell_ref's walkers; the partner atoms are appended BEHIND shell_ref's items (so
neither list of the shell sees them) at the anchor plus small dyadic offsets along ONE axis per (vector, frame), the axis and
the sign drawn from a seeded integer pattern:

    bond      d_ab = sign s e_i
    bisector  d_ab = sign s (e_i + e_j),  d_ac = sign s (e_i - e_j)          -> v = 2 sign s e_i
    normal    d_ab = sign s e_i,          d_ac = s e_j                       -> v = sign s^2 e_k        (i, j, k cyclic)

so every v is along an axis, every component of u is exactly -1, 0 or 1 in float64 as in the integers here (the reference
works in INTEGER grid units and asserts that v has at most one non-zero component), c is -1, 0 or 1, and S is an exact
integer, asserted below 2^53: EVERY comparison is for equality.  In boxed cases some partners are moved through a face by a
whole box length of their frame (powers of two: exact), so the image step has work to do; the reference asserts that every
difference it has unwrapped is shorter than half the box.  `zero` marks (vector, frame) entries whose atoms coincide: v = 0."""
import functools

import numpy as np

import shell_msd_ref as mref
import shell_ref

GRID = shell_ref.GRID
CONDITIONS = mref.CONDITIONS
MODES = ("bond", "bisector", "normal")
ROW_LEN = {"bond": 2, "bisector": 3, "normal": 3}


def unit_vectors(x, rows, mode, box):
    """u (N, T, 3) int64 with components in {-1, 0, 1}.  x (T, A, 3) on the grid; rows (N, K) atoms; box None or (T, 3)"""
    xi = shell_ref.grid_units(x, "a position")
    T = xi.shape[0]
    rows = np.asarray(rows)
    assert rows.shape[1] == ROW_LEN[mode]
    Hi = None
    if box is not None:
        box = np.broadcast_to(np.asarray(box, dtype=np.float64), (T, 3))
        assert np.all(np.frexp(box)[0] == 0.5), "the box lengths must be powers of two"
        Hi = shell_ref.grid_units(box, "a box length")[:, None, :]

    def diff(j):
        d = xi[:, rows[:, j]] - xi[:, rows[:, 0]]  # (T, N, 3)
        if Hi is not None:
            d = d - np.rint(d / Hi).astype(np.int64) * Hi
            assert np.all(2 * np.abs(d) < Hi), "an unwrapped difference is not below half the box"
        assert np.abs(d).max(initial=0) < 2 ** 20
        return d

    db = diff(1)
    if mode == "bond":
        v = db
    elif mode == "bisector":
        v = db + diff(2)
    else:
        v = np.cross(db, diff(2))
    assert np.all((v != 0).sum(axis=2) <= 1), "a vector is not along an axis"
    return np.sign(v).transpose(1, 0, 2)


def gated_sums(u, g, L, condition):
    """(S (L + 1, 2) float64, N (L + 1,) int64) of u (N, T, 3) with integer components and g (N, T) bool"""
    u = np.asarray(u, dtype=np.int64)
    g = np.asarray(g, dtype=bool)
    N_, T, _ = u.shape
    assert g.shape == (N_, T) and 0 <= L <= T - 1 and condition in CONDITIONS
    S = np.zeros((L + 1, 2), dtype=np.int64)
    N = np.zeros(L + 1, dtype=np.int64)
    w = g.copy()
    for tau in range(L + 1):
        if tau:
            w = (w[:, :-1] & g[:, tau:]) if condition == "continuous" else (g[:, :T - tau] & g[:, tau:])
        c = (u[:, :T - tau] * u[:, tau:]).sum(axis=2)
        assert np.abs(c).max(initial=0) <= 1
        S[tau] = (c * w).sum(), (c * c * w).sum()
        N[tau] = w.sum()
    assert np.abs(S).max(initial=0) < 2 ** 53
    return S.astype(np.float64), N


def with_partners(x, b, mode, anchor, box, seed, zero=None, wrap=0.3):
    """(x' (T, A + N (K - 1), 3), rows (N, K)): the partner atoms of the anchors b appended behind x's items, row n with b[n]
    in column `anchor` (see the module text).  box: None or (T, 3): partners go through a face with probability `wrap`.
    zero: None or (N, T) bool: all atoms of the row on the anchor"""
    x = np.asarray(x, dtype=np.float64)
    T, A, _ = x.shape
    b = np.asarray(b)
    N, K = b.size, ROW_LEN[mode]
    assert 0 <= anchor < K
    rng = np.random.default_rng(seed + 77)
    axis = rng.integers(0, 3, size=(N, T))
    # (the axis changes now and then, not in every frame: c = 1 and c = 0 both occur at every lag)
    keep = rng.random((N, T)) < 0.8
    for t in range(1, T):
        axis[:, t] = np.where(keep[:, t], axis[:, t - 1], axis[:, t])
    sign = rng.choice([-1.0, 1.0], size=(N, T))
    s = rng.choice([0.25, 0.5], size=(N, T))
    e = np.eye(3)
    ei, ej = e[axis], e[(axis + 1) % 3]  # (N, T, 3)
    rel = np.zeros((K, N, T, 3))  # the row's atoms relative to its first atom
    if mode == "bond":
        rel[1] = (sign * s)[..., None] * ei
    elif mode == "bisector":
        rel[1] = (sign * s)[..., None] * (ei + ej)
        rel[2] = (sign * s)[..., None] * (ei - ej)
    else:
        rel[1] = (sign * s)[..., None] * ei
        rel[2] = s[..., None] * ej
    if zero is not None:
        rel[:, np.asarray(zero, dtype=bool)] = 0.0
    rel = rel - rel[anchor][None]  # ... and to the anchor
    out = np.concatenate([x, np.zeros((T, N * (K - 1), 3))], axis=1)
    rows = np.zeros((N, K), dtype=np.int32)
    rows[:, anchor] = b
    others = [j for j in range(K) if j != anchor]
    for m, j in enumerate(others):
        ids = A + m * N + np.arange(N)
        rows[:, j] = ids
        p = x[:, b] + rel[j].transpose(1, 0, 2)
        if box is not None:
            H = np.broadcast_to(np.asarray(box, dtype=np.float64), (T, 3))[:, None, :]
            p = p + rng.choice([-1.0, 0.0, 1.0], p=[wrap / 2, 1 - wrap, wrap / 2], size=p.shape) * H
        out[:, ids] = p
    assert np.array_equal(out, out.astype(np.float32).astype(np.float64)), "float32 staging must be lossless"
    return out, rows


@functools.lru_cache(maxsize=None)
def case(T, Na, Nb, kind, boxed, gap, L, mode, anchor=0, seed=1):
    """shell_ref.case (D = 3) with partner atoms: (x, a, b, rows, dims, axes, cuts, g, {condition: (S, N)}, runs, nb), computed
    once and shared; not to be modified.  kind "same": a = the Nb items, b = None (the anchors are the reference list)"""
    x, a, b, dims, axes, cuts, s, (ci, runs, nb, cc) = shell_ref.case(T, Na, Nb, 3, kind, boxed, gap, seed)
    anchors = np.arange(Nb) if b is None else b
    if kind == "same":
        a = np.arange(Nb)
    box = None if dims is None else dims[:, :3]
    x2, rows = with_partners(x, anchors, mode, anchor, box, seed)
    g = shell_ref.filtered(s, gap)
    assert np.array_equal(shell_ref.levels(x2, a, b, box, **cuts), s)  # (the partners are no items of the shell)
    u = unit_vectors(x2, rows, mode, box)
    want = {}
    for condition in CONDITIONS:
        S, N = gated_sums(u, g, L, condition)
        r, n = mref.check_counts(g, L, N, condition)
        assert np.array_equal(r, runs) and np.array_equal(n, nb)
        S.setflags(write=False), N.setflags(write=False)
        want[condition] = (S, N)
    x2.setflags(write=False), rows.setflags(write=False)
    return x2, a, b, rows, dims, axes, cuts, g, want, runs, nb


def float_sums(x, rows, mode, box, g, L, condition):
    """(S (L + 1, 2), N) by a float64 NumPy evaluation of the definition for positions that are on no grid"""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    rows = np.asarray(rows)

    def diff(j):
        d = x[:, rows[:, j]] - x[:, rows[:, 0]]
        if box is not None:
            H = np.broadcast_to(np.asarray(box, dtype=np.float64), (T, 3))[:, None, :]
            d = d - np.rint(d / H) * H
        return d

    db = diff(1)
    v = db if mode == "bond" else db + diff(2) if mode == "bisector" else np.cross(db, diff(2))
    n = np.sqrt((v * v).sum(axis=2, keepdims=True))
    u = np.where(n > 0, v / np.where(n > 0, n, 1.0), 0.0).transpose(1, 0, 2)
    S = np.zeros((L + 1, 2))
    N = np.zeros(L + 1, dtype=np.int64)
    w = g.copy()
    for tau in range(L + 1):
        if tau:
            w = (w[:, :-1] & g[:, tau:]) if condition == "continuous" else (g[:, :T - tau] & g[:, tau:])
        c = (u[:, :T - tau] * u[:, tau:]).sum(axis=2)
        S[tau] = (c * w).sum(), (c * c * w).sum()
        N[tau] = w.sum()
    return S, N
