"""Long-double reference of the rotational correlation functions, written from the definitions of include/ta_hip.h
(ta_orient) and independent of the library:

    d(a -> b) = x[t, b] - x[t, a], with a box reduced by one sequential image step per axis (z, y, x) against the rows of H
                and the diagonal of M = H^-1 (H by MDAnalysis' triclinic_vectors formula in float64, as the header says)
    v         = d(a -> b) | d(a -> b) + d(a -> c) | d(a -> b) x d(a -> c);   u = v / |v|, 0 for a vector without a direction
    c1[tau]   = 1/(T - tau) sum_{t < T - tau} sum_n P1(u_n(t) . u_n(t + tau)),          P1(c) = c
    c2[tau]   = 1/(T - tau) sum_{t < T - tau} sum_n P2(u_n(t) . u_n(t + tau)),          P2(c) = (3 c^2 - 1) / 2
    total[t]  = sum_n w_n u_n(t);   coll[tau] = 1/(T - tau) sum_{t < T - tau} total[t] . total[t + tau]

P2 is formed directly, not through Q; the library's c2 is 2/3 of it (it returns sum Q : Q').  A degenerate vector contributes
nothing to any sum.  x: the float64 values actually staged.  The lag sums are direct sums at lag_sample(T).

The inputs are molecules of three atoms (a, b, c): a walks on a 1/1024 grid (exact in float32), b and c sit 0.6 ... 1.4 length
units from it in slowly turning directions, in boxes of at least 12: the minimum-image condition holds, and the generator
asserts on the CPU that no rint argument of the image step comes within 0.01 of a half."""
import functools

import numpy as np

from scatter_ref import lag_sample  # noqa: F401  (the project's lag sample, shared)

LD = np.longdouble
U_R = 2.0 ** -53
MODES = ("bond", "bisector", "normal")


def box_matrix(dims):
    """H (rows: the box vectors, lower-triangular) of [a, b, c, alpha, beta, gamma] in float64, MDAnalysis' formula"""
    a, b, c, al, be, ga = (float(v) for v in dims)
    H = np.zeros((3, 3))
    if al == 90.0 and be == 90.0 and ga == 90.0:
        H[0, 0], H[1, 1], H[2, 2] = a, b, c
        return H
    ca, cb, cg = (0.0 if v == 90.0 else np.cos(np.deg2rad(v)) for v in (al, be, ga))
    sg = 1.0 if ga == 90.0 else np.sin(np.deg2rad(ga))
    H[0, 0] = a
    H[1, 0], H[1, 1] = b * cg, b * sg
    H[2, 0] = c * cb
    H[2, 1] = c * (ca - cb * cg) / sg
    H[2, 2] = np.sqrt(c * c - H[2, 0] ** 2 - H[2, 1] ** 2)
    return H


def boxes(dimensions, T):
    """(T, 3, 3) H per frame of a (6,) or (T, 6) dimensions array"""
    d = np.asarray(dimensions, dtype=np.float64)
    if d.ndim == 1:
        d = np.broadcast_to(d, (T, 6))
    return np.stack([box_matrix(r) for r in d])


def image(d, H, margin=None):
    """the sequential image step of long-double differences d (T, N, 3) with H (T, 3, 3) float64; margin: a one-element list
    that receives the smallest distance of a rint argument from a half"""
    d = np.array(d, dtype=LD)
    for j in (2, 1, 0):
        m = (1.0 / H[:, j, j]).astype(LD)[:, None]  # the float64 reciprocal, as the table holds it
        sc = d[:, :, j] * m
        k = np.rint(sc)
        if margin is not None:
            margin[0] = min(margin[0], float(np.min(np.abs(np.abs(sc - np.floor(sc)) - 0.5))))
        for i in range(j + 1):
            d[:, :, i] = d[:, :, i] - k * H[:, j, i].astype(LD)[:, None]
    return d


def unit_vectors(x, index, mode, dimensions=None, margin=None):
    """(T, N, 3) long-double u (zeros for a degenerate vector) of the staged values x (T, A, 3)"""
    x = np.asarray(x, dtype=LD)
    idx = np.asarray(index)
    T = x.shape[0]
    H = None if dimensions is None else boxes(dimensions, T)
    diff = lambda j: x[:, idx[:, j]] - x[:, idx[:, 0]]
    db = diff(1) if H is None else image(diff(1), H, margin)
    if mode == "bond":
        v = db
    else:
        dc = diff(2) if H is None else image(diff(2), H, margin)
        v = db + dc if mode == "bisector" else np.cross(db, dc)
    n = np.sqrt((v * v).sum(axis=2))
    ok = n > 0
    return np.where(ok[:, :, None], v / np.where(ok, n, 1)[:, :, None], LD(0))


def lag_sums(u, lags):
    """(c1, c2) at `lags`: the direct sums of P1 and P2 over the non-degenerate vectors"""
    T = u.shape[0]
    live = (u * u).sum(axis=2) > 0
    c1, c2 = np.zeros(len(lags), dtype=LD), np.zeros(len(lags), dtype=LD)
    for i, tau in enumerate(lags):
        n = T - int(tau)
        c = (u[:n] * u[int(tau):]).sum(axis=2)
        both = live[:n] & live[int(tau):]
        c1[i] = c.sum() / n
        c2[i] = (np.where(both, (3 * c * c - 1) / 2, LD(0))).sum() / n
    return c1, c2


def coll_at(total, lags):
    """the long-double autocorrelation of a (T, 3) total (e.g. the one a call returned) at `lags`"""
    m = np.asarray(total, dtype=LD)
    T = m.shape[0]
    return np.array([(m[:T - int(k)] * m[int(k):]).sum() / (T - int(k)) for k in lags], dtype=LD)


def total_bar(n_vectors, weights, ratio):
    """(B_u + 1 + N) 2^-53 sum |w|, B_u = 12 + 3 R: the header's bound on a component of the total (R 0 without a box)"""
    sw = float(n_vectors) if weights is None else float(np.sum(np.abs(weights)))
    return (12.0 + 3.0 * ratio + 1.0 + n_vectors) * U_R * sw


def molecules(T, n_mol, seed, box=12.0):
    """(T, 3 n_mol, 3) float64 positions on a 1/1024 grid: atom 3 m a walker around the middle of a box of `box`, atoms
    3 m + 1 and 3 m + 2 at 0.6 ... 1.4 from it, about 104 degrees apart, the molecule tumbling"""
    rng = np.random.default_rng(seed)
    steps = np.rint(rng.normal(scale=0.05 * 1024, size=(T, n_mol, 3)))
    start = np.rint(rng.uniform(0.25 * box, 0.75 * box, size=(1, n_mol, 3)) * 1024)
    a = (np.cumsum(steps, axis=0) + start) / 1024.0
    # a tumbling orthonormal frame per molecule: random-walk rotation vectors, Rodrigues
    w = np.cumsum(rng.normal(scale=0.15, size=(T, n_mol, 3)), axis=0) + rng.uniform(-3, 3, size=(1, n_mol, 3))
    ang = np.linalg.norm(w, axis=2, keepdims=True)
    k = w / ang

    def rot(v):
        return v * np.cos(ang) + np.cross(k, v) * np.sin(ang) + k * (k * v).sum(axis=2, keepdims=True) * (1 - np.cos(ang))

    half = np.deg2rad(52.0)
    rb = rng.uniform(0.75, 1.3, size=(1, n_mol, 1))
    rc = rng.uniform(0.75, 1.3, size=(1, n_mol, 1))
    e1 = np.broadcast_to(np.array([np.cos(half), np.sin(half), 0.0]), (T, n_mol, 3))
    e2 = np.broadcast_to(np.array([np.cos(half), -np.sin(half), 0.0]), (T, n_mol, 3))
    b = a + np.rint(rb * rot(e1) * 1024) / 1024.0
    c = a + np.rint(rc * rot(e2) * 1024) / 1024.0
    x = np.stack([a, b, c], axis=2).reshape(T, 3 * n_mol, 3)
    for p in (b, c):
        r = np.linalg.norm(p - a, axis=2)
        assert r.min() >= 0.6 and r.max() <= 1.4, (r.min(), r.max())
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    return x


def index_rows(n_vectors, n_mol, mode, seed):
    """n_vectors rows over the molecules' atoms, in a permuted order, the centre atom a first; with more vectors than
    molecules atoms are shared between vectors (bond: (a, b) and (a, c) of a molecule; else (a, b, c) and (a, c, b))"""
    m = np.arange(n_vectors) % n_mol
    alt = (np.arange(n_vectors) // n_mol) % 2
    b, c = 3 * m + 1 + alt, 3 * m + 2 - alt
    rows = np.stack([3 * m, b] if mode == "bond" else [3 * m, b, c], axis=1)
    return np.ascontiguousarray(rows[np.random.default_rng(seed + 7).permutation(n_vectors)], dtype=np.int32)


def wrap(x, dimensions):
    """x wrapped into the box(es) atom by atom: x - floor(x H^-1) H, float64"""
    T = x.shape[0]
    H = boxes(dimensions, T)
    out = np.array(x, dtype=np.float64)
    for j in (2, 1, 0):
        n = np.floor(out[:, :, j] / H[:, j, j][:, None])
        for i in range(j + 1):
            out[:, :, i] -= n * H[:, j, i][:, None]
    return out


def near_corner_wrapped(x, index, box, seed=9):
    """case()'s molecules (every molecule the centre of one vector) moved to within 0.4 of the box's origin corner and on by
    whole box vectors, then wrapped into the box(es) `box` (T, 6) atom by atom: the faces cut through many of them"""
    T, A = x.shape[:2]
    idx = np.asarray(index)
    mol = np.arange(A) // 3
    mol[[1, A - 1]] = mol[[A - 1, 1]]  # (case() keeps the first molecule's b in the last slot of the slab)
    rng = np.random.default_rng(seed)
    centre = x[0, idx[np.argsort(mol[idx[:, 0]], kind="stable"), 0]][:A // 3]  # atom a of molecule 0, 1, ...
    near = np.rint((rng.uniform(-0.4, 0.4, size=centre.shape) - centre) * 1024) / 1024.0
    images = rng.integers(-2, 3, size=(A // 3, 3)).astype(np.float64)
    far = x + near[mol][None] + np.einsum("ni,tij->tnj", images[mol], boxes(box, T))
    wrapped = wrap(far, box)
    cut = np.abs(wrapped[:, idx[:, 1]] - wrapped[:, idx[:, 0]]).max(axis=2) > 2.0
    assert cut.any() and not cut.all()  # some vectors are cut by a face in some frames
    return wrapped


ORTHO = (12.0, 13.5, 16.0, 90.0, 90.0, 90.0)   # dyadic lengths: wrapped positions stay on the 1/1024 grid
TRIC = (13.0, 14.0, 15.0, 75.0, 80.0, 70.0)


def box_frames(dims, T, moving):
    """(T, 6): the box constant, or (moving) breathing by up to 2 percent from frame to frame (lengths only)"""
    d = np.tile(np.asarray(dims, dtype=np.float64), (T, 1))
    if moving:
        d[:, :3] *= (1.0 + 0.02 * np.sin(0.3 * np.arange(T)))[:, None]
    return d


def check_image_conditions(x, index, mode, dimensions):
    """the generator's two conditions, on the CPU: every vector's arms are shorter than half the smallest box width, and no
    rint argument of the image step is within 0.01 of a half.  -> R of total_bar: the largest raw difference component over
    the smallest |v|"""
    T = x.shape[0]
    H = boxes(dimensions, T)
    widths = np.stack([1.0 / np.linalg.norm(np.linalg.inv(h), axis=0) for h in H])  # distance between opposite faces
    margin = [1.0]
    idx = np.asarray(index)
    longest, raw = 0.0, 0.0
    xl = np.asarray(x, dtype=LD)
    for j in range(1, idx.shape[1]):
        d0 = xl[:, idx[:, j]] - xl[:, idx[:, 0]]
        d = image(d0, H, margin)
        longest = max(longest, float(np.sqrt((d * d).sum(axis=2)).max()))
        raw = max(raw, float(np.abs(d0).max()))
    assert longest < 0.5 * widths.min(), (longest, widths.min())
    assert margin[0] >= 0.01, margin[0]
    return raw / 0.5  # |v| >= 0.5 for every mode of these molecules (molecules(): arms >= 0.75 - a grid step, 104 degrees apart)


def reference(x, index, mode, dimensions=None, weights=None):
    """(lags, c1, c2, total, bar, sum |w|): the long-double reference of one call, and the bound on a component of the total"""
    x = np.asarray(x, dtype=np.float64)
    T, N = x.shape[0], len(index)
    ratio = 0.0
    if dimensions is not None:
        ratio = check_image_conditions(x, index, mode, dimensions)
    lags = lag_sample(T)
    u = unit_vectors(x, index, mode, dimensions)
    c1, c2 = lag_sums(u, lags)
    w = np.ones(N, dtype=LD) if weights is None else np.asarray(weights, dtype=LD)
    total = (u * w[None, :, None]).sum(axis=1)
    return lags, c1, c2, total, total_bar(N, weights, ratio), float(np.abs(w).sum())


@functools.lru_cache(maxsize=64)
def case(T, N, mode, seed=1, weighted=False, n_mol=None):
    """(x float64 (exact in float32), index, weights or None, reference(...) without a box): computed once and shared; not
    to be modified.  n_mol: molecules in the slab (default: N, every molecule one vector)"""
    n_mol = n_mol or N
    x = molecules(T, n_mol, seed)
    x[:, [1, 3 * n_mol - 1]] = x[:, [3 * n_mol - 1, 1]]  # the first molecule's b is the LAST atom of the slab
    idx = index_rows(N, n_mol, mode, seed)
    swap = {1: 3 * n_mol - 1, 3 * n_mol - 1: 1}
    idx = np.vectorize(lambda i: swap.get(int(i), int(i)), otypes=[np.int32])(idx)
    w = np.random.default_rng(seed + 3).uniform(-1.5, 1.5, size=N) if weighted else None
    ref = reference(x, idx, mode, None, w)
    for a in (x, idx) + ((w,) if w is not None else ()) + tuple(ref[:4]):
        a.setflags(write=False)
    return x, idx, w, ref


def assert_orient(got, ref, what=""):
    """The four outputs (c1, c2, total, coll; None: not asked for) of a call against reference(...): c1 and 1.5 c2 within
    1e-10 of their maxima at the lags, the total within its derived bar (itself at most 1e-10 sum |w|), coll within 1e-10 of
    its maximum against the long-double autocorrelation of the RETURNED total; every figure printed before it is asserted."""
    lags, c1, c2, total, bar, sw = ref
    g1, g2, gt, gc = got
    for name, g, want, f in (("c1", g1, c1, 1.0), ("c2", g2, c2, 1.5)):
        if g is None:
            continue
        scale = float(np.max(np.abs(want)))
        err = float(np.max(np.abs(f * np.asarray(g, dtype=LD)[lags] - want))) / scale
        print(f"    {what} {name}: {err:.3e} of {scale:.3e}")
        assert err <= 1e-10, (what, name, err)
    if gt is not None:
        err = float(np.max(np.abs(np.asarray(gt, dtype=LD) - total)))
        print(f"    {what} total: {err:.3e} (bar {bar:.3e}, 1e-10 sum |w| = {1e-10 * sw:.3e})")
        assert bar <= 1e-10 * sw, (what, bar, sw)
        assert err <= bar, (what, err, bar)
    if gc is not None:
        want = coll_at(gt, lags)
        scale = float(np.max(np.abs(want)))
        err = float(np.max(np.abs(np.asarray(gc, dtype=LD)[lags] - want))) / (scale if scale > 0 else 1.0)
        print(f"    {what} coll: {err:.3e} of {scale:.3e}")
        assert err <= 1e-10, (what, err)
