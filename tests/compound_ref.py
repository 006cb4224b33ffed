"""Reference for ta_compound, and the inputs and plans its tests share.  Nothing here is shared with the library.

    out[t, c, d] = sum_{i in compound c} w_i x[t, m_i, d]  -  g_c F[t, d],     g_c = sum_i w_i,   F[t, d] = sum_a u_a x[t, a, d]

Every product w x (and u x) is formed in float64, as the library forms it; the terms are ADDED in NumPy long double, g_c F
is formed in long double, and the result is rounded to float64 once.

The bar is derived, not tuned.  The library adds the k_c terms of a compound in float64 (the first product, then one fma per
term) and F's A terms in some fixed order; the standard bound of such a sum is gamma_n sum |terms| with gamma_n ~ n 2^-53.
Twice that for both parts, per element:

    |got - want| <= 2^-52 ( k_c sum_i |w_i x_i(t)|  +  |g_c| A sum_a |u_a x_a(t)| )

which also covers the one rounding of g_c (k_c terms), the final fma and the reference's own rounding."""
import functools

import numpy as np

LD = np.longdouble


def compound_ref(x, offsets, members, weights=None, frame_weights=None):
    """(want, bar): both (T, C, D) float64"""
    x = np.asarray(x, dtype=np.float64)
    T, A, D = x.shape
    offsets = np.asarray(offsets, dtype=np.int64)
    members = np.asarray(members, dtype=np.int64)
    w = np.ones(members.size) if weights is None else np.asarray(weights, dtype=np.float64)
    k = np.diff(offsets)
    terms = x[:, members, :] * w[None, :, None]  # float64 products
    want = np.add.reduceat(terms.astype(LD), offsets[:-1], axis=1)
    mag = np.add.reduceat(np.abs(terms), offsets[:-1], axis=1)
    bar = k[None, :, None] * mag
    if frame_weights is not None:
        u = np.asarray(frame_weights, dtype=np.float64)
        fterms = x * u[None, :, None]
        F = fterms.astype(LD).sum(axis=1)  # (T, D)
        g = np.add.reduceat(w.astype(LD), offsets[:-1])
        want = want - g[None, :, None] * F[:, None, :]
        bar = bar + np.abs(g.astype(np.float64))[None, :, None] * A * np.abs(fterms).sum(axis=1)[:, None, :]
    return want.astype(np.float64), 2.0 ** -52 * bar


def assert_compound(got, want, bar, what=""):
    """every element within its bar; prints the worst ratio before it asserts (an element whose bar is 0 must be exact)"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"    compound {what}: worst |got - want| / bar = {worst:.3e}")
    assert worst <= 1.0, f"{what}: {worst:.3e} of the derived bar"


def positions(T, A, D, seed):
    """random walks some hundred away from the origin, like unwrapped positions in a box, rounded to float32 first so that
    a float64 and a float32 slab hold the same values"""
    rng = np.random.default_rng(seed)
    x = 300.0 * rng.random((1, A, D)) + np.cumsum(0.05 * rng.standard_normal((T, A, D)), axis=0)
    return x.astype(np.float32).astype(np.float64)


def masses(A, seed):
    return np.random.default_rng(seed + 1).choice([1.008, 12.011, 14.007, 15.999, 18.998, 32.06], size=A)


def plan_mixed(A, odd, skip=5):
    """contiguous members: compounds of 1, 2, 3 and 15 atoms in turn and ONE of 300 (under 700 atoms: of 40) in the middle of the
    plan; the last `skip` atoms are named by no compound.  `odd`: the parity of the compound count."""
    big_n = 300 if A >= 700 else 40  # (the host-sized cases)
    sizes, used, big = [], 0, A >= 100
    cycle = (1, 2, 3, 15)
    i = 0
    while True:
        n = big_n if big and used >= (A - big_n) // 2 else cycle[i % 4]
        if used + n > A - skip:
            break
        if n == big_n:
            big = False
        else:
            i += 1
        sizes.append(n)
        used += n
    if len(sizes) % 2 != int(odd):
        sizes.pop()
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return offsets, np.arange(offsets[-1], dtype=np.int32)


def plan_interleaved(A, C, skip=5):
    """atom n in compound n % C, for the atoms below A - skip: with dim = 3 every straddling source pair holds two compounds"""
    n = np.arange(A - skip)
    order = np.argsort(n % C, kind="stable")
    counts = np.bincount(n % C, minlength=C)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return offsets, order.astype(np.int32)


def normalised(offsets, members, m):
    """the members' masses / their compound's mass"""
    w = np.asarray(m, dtype=np.float64)[members]
    total = np.add.reduceat(w, offsets[:-1])
    return w / np.repeat(total, np.diff(offsets))


@functools.lru_cache(maxsize=4)
def compound_case(T, A, D, kind, odd):
    """(x, offsets, members, weights, u, (want, bar) without the frame term, (want, bar) with it), read-only.
    kind "mixed": plan_mixed; "inter": plan_interleaved with 100 (under 1000 atoms: 12) compounds, one more when odd."""
    x = positions(T, A, D, seed=T + A + D)
    m = masses(A, seed=A)
    offsets, members = plan_mixed(A, odd) if kind == "mixed" else plan_interleaved(A, (100 if A >= 1000 else 12) + int(odd))
    assert (offsets.size - 1) % 2 == int(odd)
    w = normalised(offsets, members, m)
    u = m / m.sum()
    plain = compound_ref(x, offsets, members, w)
    framed = compound_ref(x, offsets, members, w, u)
    for a in (x, offsets, members, w, u, *plain, *framed):
        a.setflags(write=False)
    return x, offsets, members, w, u, plain, framed
