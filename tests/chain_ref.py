"""Long-double reference of the chain functionals, written from the definitions of include/ta_hip.h (ta_chain_modes) and
independent of the library:

    s_1 = 0,  s_n = s_{n-1} + img(x[t, m_n] - x[t, m_{n-1}]),  with a box img = one sequential image step per axis (z, y, x)
              against the rows of H and the diagonal of M = H^-1 (H by MDAnalysis' triclinic_vectors formula in float64, the
              float64 reciprocal of its diagonal: orient_ref's image(), which restates exactly that)
    Y_q(c, t) = sum_{n = 2 ... N} coeff[q][n - 1] s_n
    acf[q][tau] = 1/(T - tau) sum_{t < T - tau} sum_c Y_q(c, t) . Y_q(c, t + tau)           (not divided by n_chains)

x: the float64 values actually staged (for a float32 slab the float32-rounded values).  The lag sums are direct sums at
lag_sample(T).  The bar is the library's standing one: every series within 1e-10 of its own maximum.

The inputs are chains of beads on a 1/1024 grid (exact in float32) with bonds of 0.6 ... 1.4 length units whose directions
turn slowly, in boxes of at least 12: the minimum-image condition holds with room, and reference() asserts on the CPU that no
rint argument of the image step comes within 0.01 of a half."""
import functools

import numpy as np

from orient_ref import ORTHO, TRIC, box_frames, boxes, image, wrap  # noqa: F401  (the box restatement, shared)
from scatter_ref import lag_sample  # noqa: F401  (the project's lag sample, shared)

LD = np.longdouble
BAR = 1e-10


def rouse_coeff(N, modes):
    """(len(modes), N) float64: cos(p pi (n - 1/2) / N) / N, n = 1 ... N"""
    n = np.arange(1, N + 1, dtype=np.float64)[None, :]
    p = np.asarray(modes, dtype=np.float64)[:, None]
    return np.cos(p * np.pi * (n - 0.5) / N) / N


def end_to_end_row(N):
    e = np.zeros((1, N))
    e[0, -1] = 1.0
    return e


def whole_chains(x, members, dimensions=None, margin=None):
    """(T, C, N, 3) long-double s of the staged values x (T, A, 3): every chain relative to its first bead"""
    x = np.asarray(x, dtype=LD)
    m = np.asarray(members)
    T = x.shape[0]
    C, N = m.shape
    r = x[:, m.ravel()].reshape(T, C, N, 3)
    d = (r[:, :, 1:] - r[:, :, :-1]).reshape(T, C * (N - 1), 3)
    if dimensions is not None:
        d = image(d, boxes(dimensions, T), margin)
    s = np.zeros((T, C, N, 3), dtype=LD)
    s[:, :, 1:] = np.cumsum(d.reshape(T, C, N - 1, 3), axis=2)
    return s


def functionals(x, members, coeff, dimensions=None, margin=None):
    """(Q, T, C, 3) long-double Y"""
    s = whole_chains(x, members, dimensions, margin)
    return np.einsum("qn,tcnd->qtcd", np.asarray(coeff, dtype=LD), s)


def lag_sums(Y, lags):
    """(Q, len(lags)) long double: the direct sums"""
    T = Y.shape[1]
    out = np.zeros((Y.shape[0], len(lags)), dtype=LD)
    for i, tau in enumerate(lags):
        n = T - int(tau)
        out[:, i] = (Y[:, :n] * Y[:, int(tau):]).sum(axis=(1, 2, 3)) / n
    return out


def reference(x, members, coeff, dimensions=None):
    """(lags, acf (Q, len(lags)) long double) of one call; with a box, the generator's two conditions are asserted: every bond
    shorter than half the smallest box width, no rint argument within 0.01 of a half"""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    margin = [1.0]
    Y = functionals(x, members, coeff, dimensions, margin)
    if dimensions is not None:
        H = boxes(dimensions, T)
        widths = np.stack([1.0 / np.linalg.norm(np.linalg.inv(h), axis=0) for h in H])
        s = whole_chains(x, members, dimensions)
        bonds = np.sqrt(((s[:, :, 1:] - s[:, :, :-1]) ** 2).sum(axis=3).astype(np.float64))
        assert bonds.max() < 0.5 * widths.min(), (bonds.max(), widths.min())
        assert margin[0] >= 0.01, margin[0]
    lags = lag_sample(T)
    return lags, lag_sums(Y, lags)


def assert_chain(got, want, what=""):
    """acf (Q, T) of a call against reference(...): every row within 1e-10 of its own maximum at the lags; a row whose reference
    is identically zero must be exactly zero.  Every figure is printed before it is asserted."""
    lags, acf = want
    got = np.asarray(got)
    assert got.shape[0] == acf.shape[0] and np.all(np.isfinite(got)), (what, got.shape)
    for q in range(acf.shape[0]):
        scale = float(np.max(np.abs(acf[q])))
        if scale == 0.0:
            assert not got[q].any(), (what, q, "a zero functional must give exact zeros")
            continue
        err = float(np.max(np.abs(got[q].astype(LD)[lags] - acf[q]))) / scale
        print(f"    {what} functional {q}: {err:.3e} of {scale:.3e}")
        assert err <= BAR, (what, q, err)


def chain_coordinates(T, C, N, seed, box=12.0):
    """(T, C, N, 3) float64 on a 1/1024 grid: chain c starts at a slowly diffusing bead around the middle of a box of `box`,
    every further bead 0.6 ... 1.4 from the one before in a direction that turns slowly"""
    rng = np.random.default_rng(seed)
    steps = np.rint(rng.normal(scale=0.03 * 1024, size=(T, C, 1, 3)))
    start = np.rint(rng.uniform(0.3 * box, 0.7 * box, size=(1, C, 1, 3)) * 1024)
    first = (np.cumsum(steps, axis=0) + start) / 1024.0
    v = rng.normal(size=(1, C, N - 1, 3)) + np.cumsum(rng.normal(scale=0.08, size=(T, C, N - 1, 3)), axis=0)
    v /= np.linalg.norm(v, axis=3, keepdims=True)
    length = rng.uniform(0.75, 1.3, size=(1, C, N - 1, 1))
    bonds = np.rint(length * v * 1024) / 1024.0
    r = np.concatenate([first, first + np.cumsum(bonds, axis=2)], axis=2)
    b = np.linalg.norm(bonds, axis=3)
    assert b.min() >= 0.6 and b.max() <= 1.4, (b.min(), b.max())
    assert np.array_equal(r, r.astype(np.float32).astype(np.float64))
    return r


def member_table(C, N, layout, seed=0):
    """(C, N) int32 over the atoms 0 ... C N - 1: "blocked" chain c = atoms c N ... c N + N - 1; "interleaved" chain c = atoms
    c, c + C, ...; "permuted" a random assignment of atoms to beads (chains start on odd and on even atoms, the chain list in no
    order)"""
    if layout == "blocked":
        m = np.arange(C * N).reshape(C, N)
    elif layout == "interleaved":
        m = np.arange(C * N).reshape(N, C).T
    else:
        m = np.random.default_rng(seed + 11).permutation(C * N).reshape(C, N)
    return np.ascontiguousarray(m, dtype=np.int32)


def place(r, members):
    """the slab (T, A, 3) that holds bead n of chain c at atom members[c, n]"""
    T, C, N, _ = r.shape
    x = np.zeros((T, C * N, 3))
    x[:, np.asarray(members).ravel()] = r.reshape(T, C * N, 3)
    return x


def cut_wrapped(x, members, dimensions, shift=-5.0, need_cut=True):
    """x moved by `shift` along every axis (chain_coordinates' chains then lie around the box's origin corner) and wrapped into
    the box(es) (T, 6) atom by atom: the faces cut through many of the chains"""
    m = np.asarray(members)
    wrapped = wrap(np.asarray(x) + shift, dimensions)
    r = wrapped[:, m.ravel()].reshape(x.shape[0], m.shape[0], m.shape[1], 3)
    cut = np.abs(r[:, :, 1:] - r[:, :, :-1]).max(axis=3) > 3.0
    if need_cut:
        assert cut.any() and not cut.all()  # some bonds are cut by a face in some frames
    return wrapped


def mixed_coeff(N, Q, seed=0, zero_rows=()):
    """(Q, N) rows: Rouse modes 1, 2, ... while they exist (p <= N - 1), then the end-to-end row, then random rows; the rows in
    `zero_rows` all zero"""
    rng = np.random.default_rng(seed + 5)
    rows = []
    for q in range(Q):
        if q < N - 1:
            rows.append(rouse_coeff(N, [q + 1])[0])
        elif q == N - 1:
            rows.append(end_to_end_row(N)[0])
        else:
            rows.append(rng.uniform(-1, 1, size=N))
    co = np.array(rows)
    for q in zero_rows:
        co[q] = 0.0
    return co


@functools.lru_cache(maxsize=64)
def case(T, C, N, Q=2, layout="blocked", seed=1, zero_rows=()):
    """(x float64 (exact in float32), members, coeff, reference(...) without a box): computed once and shared; not to be
    modified"""
    r = chain_coordinates(T, C, N, seed)
    members = member_table(C, N, layout, seed)
    x = place(r, members)
    coeff = mixed_coeff(N, Q, seed, zero_rows)
    ref = reference(x, members, coeff)
    for a in (x, members, coeff) + tuple(ref):
        a.setflags(write=False)
    return x, members, coeff, ref
